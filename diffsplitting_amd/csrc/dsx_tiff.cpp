// dsx_tiff.cpp — uncompressed TIFF / BigTIFF stacks: the reader behind the Hagen configs' .tif frame files (the
// reference's imread(..., plugin='tifffile'), data/split_dataset.py:76-91) and the writer of the stitched prediction.
// Plain C++17 without a HIP include: it is part of libdsx.so and also compiles on its own (tests/tiff_san_main.cpp).
// Every offset and count taken from the file is checked against the file's size in 64-bit arithmetic before it is used.
// C ABI in include/dsx.h.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/dsx.h"

namespace dsx {
int fail(int code, const char* fmt, ...);   // the library's error state (dsx_model.cpp; a stand-alone build brings its own)
}
using dsx::fail;

namespace {
typedef unsigned long long ull;

const char* compression_name(uint64_t c) {
  switch (c) {
    case 2: return "CCITT RLE";
    case 3: return "CCITT T.4";
    case 4: return "CCITT T.6";
    case 5: return "LZW";
    case 6: case 7: return "JPEG";
    case 8: case 32946: return "Deflate";
    case 32773: return "PackBits";
    case 34925: return "LZMA";
    case 50000: return "Zstd";
    default: return "unknown scheme";
  }
}

bool mul_ok(uint64_t a, uint64_t b, uint64_t& r) {
  if (a != 0 && b > UINT64_MAX / a) return false;
  r = a * b;
  return true;
}
// [off, off + len) lies inside a file of `size` bytes
bool inside(uint64_t off, uint64_t len, uint64_t size) { return off <= size && len <= size - off; }

int type_size(unsigned type) {   // bytes of one value of a field type, 0 for types no tag read here uses
  switch (type) {
    case 1: case 2: case 6: case 7: return 1;    // BYTE, ASCII, SBYTE, UNDEFINED
    case 3: case 8: return 2;                    // SHORT, SSHORT
    case 4: case 9: case 13: return 4;           // LONG, SLONG, IFD
    case 16: case 17: case 18: return 8;         // LONG8, SLONG8, IFD8
    default: return 0;
  }
}

struct Entry { unsigned tag = 0, type = 0; uint64_t count = 0; unsigned char value[8] = {0}; };

struct Page {
  uint64_t W = 0, H = 0, S = 1, bits = 0, format = 1;
  std::vector<uint64_t> off;       // strip offsets
  std::vector<uint64_t> rows;      // rows of each strip
  std::string description;
};
}  // namespace

struct dsx_tiff {
  FILE* f = nullptr;
  std::string path;
  uint64_t size = 0;
  bool big = false, swap = false;
  std::vector<Page> pages;         // one per IFD
  int64_t n_pages = 0;             // > pages.size() only for an ImageJ contiguous stack
  bool contiguous = false;         // ImageJ: n_pages planes back to back from pages[0].off[0]
  int dtype = 0;
  uint64_t sample_bytes = 0, row_bytes = 0, page_bytes = 0;
  ~dsx_tiff() { if (f) fclose(f); }

  uint64_t u(const unsigned char* p, int n) const {   // an unsigned of n bytes in the file's byte order
    const bool file_le = (swap == !host_le());
    uint64_t v = 0;
    for (int i = 0; i < n; ++i) v |= (uint64_t)p[file_le ? i : n - 1 - i] << (8 * i);
    return v;
  }
  static bool host_le() { const uint16_t one = 1; unsigned char b; memcpy(&b, &one, 1); return b == 1; }
  int read_at(uint64_t off, void* dst, uint64_t len, const char* what) {
    if (!inside(off, len, size))
      return fail(DSX_ERR_INVALID, "%s: %s at offset %llu (%llu bytes) lies outside the file (%llu bytes): truncated or corrupt",
                  path.c_str(), what, (ull)off, (ull)len, (ull)size);
    if (fseeko(f, (off_t)off, SEEK_SET) != 0 || (len && fread(dst, 1, (size_t)len, f) != (size_t)len))
      return fail(DSX_ERR_INVALID, "%s: reading %s at offset %llu failed", path.c_str(), what, (ull)off);
    return DSX_OK;
  }
  // the values of an entry as unsigned integers (at most `limit` of them)
  int values(const Entry& e, uint64_t limit, std::vector<uint64_t>& out, const char* what) {
    const int ts = type_size(e.type);
    if (ts == 0 || e.type == 2)
      return fail(DSX_ERR_INVALID, "%s: tag %s has field type %u, not an integer type", path.c_str(), what, e.type);
    if (e.count < 1 || e.count > limit)
      return fail(DSX_ERR_INVALID, "%s: tag %s has %llu values (1..%llu expected)", path.c_str(), what, (ull)e.count, (ull)limit);
    uint64_t bytes;
    if (!mul_ok(e.count, (uint64_t)ts, bytes) || bytes > size)
      return fail(DSX_ERR_INVALID, "%s: tag %s (%llu values) is larger than the file", path.c_str(), what, (ull)e.count);
    std::vector<unsigned char> buf((size_t)bytes);
    const uint64_t inline_bytes = big ? 8 : 4;
    if (bytes <= inline_bytes) memcpy(buf.data(), e.value, (size_t)bytes);
    else {
      int rc = read_at(u(e.value, (int)inline_bytes), buf.data(), bytes, what);
      if (rc) return rc;
    }
    out.resize((size_t)e.count);
    for (uint64_t i = 0; i < e.count; ++i) out[(size_t)i] = u(buf.data() + i * ts, ts);
    return DSX_OK;
  }
  int scalar(const Entry& e, uint64_t& v, const char* what) {
    std::vector<uint64_t> t;
    int rc = values(e, 1, t, what);
    if (rc == DSX_OK) v = t[0];
    return rc;
  }
  int parse_ifd(uint64_t at, uint64_t& next, Page& pg);
  int parse();
};

int dsx_tiff::parse_ifd(uint64_t at, uint64_t& next, Page& pg) {
  const uint64_t cnt_bytes = big ? 8 : 2, ent_bytes = big ? 20 : 12, off_bytes = big ? 8 : 4;
  unsigned char head[8];
  int rc = read_at(at, head, cnt_bytes, "IFD entry count");
  if (rc) return rc;
  const uint64_t n = u(head, (int)cnt_bytes);
  uint64_t table;
  if (n < 1 || !mul_ok(n, ent_bytes, table) || !inside(at + cnt_bytes, table, size) || !inside(at + cnt_bytes + table, off_bytes, size))
    return fail(DSX_ERR_INVALID, "%s: the IFD at offset %llu declares %llu entries, which do not fit the file (%llu bytes)",
                path.c_str(), (ull)at, (ull)n, (ull)size);
  std::vector<unsigned char> raw((size_t)(table + off_bytes));
  if ((rc = read_at(at + cnt_bytes, raw.data(), raw.size(), "IFD entries"))) return rc;
  next = u(raw.data() + table, (int)off_bytes);

  uint64_t compression = 1, planar = 1, rows_per_strip = UINT64_MAX;
  std::vector<uint64_t> bits, format, counts;
  bool has_counts = false;
  for (uint64_t i = 0; i < n; ++i) {
    const unsigned char* p = raw.data() + i * ent_bytes;
    Entry e;
    e.tag = (unsigned)u(p, 2);
    e.type = (unsigned)u(p + 2, 2);
    e.count = u(p + 4, big ? 8 : 4);
    memcpy(e.value, p + (big ? 12 : 8), (size_t)off_bytes);
    switch (e.tag) {
      case 256: if ((rc = scalar(e, pg.W, "ImageWidth"))) return rc; break;
      case 257: if ((rc = scalar(e, pg.H, "ImageLength"))) return rc; break;
      case 258: if ((rc = values(e, 16, bits, "BitsPerSample"))) return rc; break;
      case 259: if ((rc = scalar(e, compression, "Compression"))) return rc; break;
      case 270: {
        if (e.type != 2 || e.count < 1 || e.count > size) break;          // not ASCII: no description
        std::vector<char> s((size_t)e.count + 1, '\0');
        if (e.count <= off_bytes) memcpy(s.data(), e.value, (size_t)e.count);
        else if ((rc = read_at(u(e.value, (int)off_bytes), s.data(), e.count, "ImageDescription"))) return rc;
        pg.description = s.data();                                         // up to the first NUL
        break;
      }
      case 273: if ((rc = values(e, size, pg.off, "StripOffsets"))) return rc; break;
      case 277: if ((rc = scalar(e, pg.S, "SamplesPerPixel"))) return rc; break;
      case 278: if ((rc = scalar(e, rows_per_strip, "RowsPerStrip"))) return rc; break;
      case 279: if ((rc = values(e, size, counts, "StripByteCounts"))) return rc; has_counts = true; break;
      case 284: if ((rc = scalar(e, planar, "PlanarConfiguration"))) return rc; break;
      case 339: if ((rc = values(e, 16, format, "SampleFormat"))) return rc; break;
      case 322: case 323: case 324: case 325: {
        uint64_t v = 0;
        std::vector<uint64_t> t;
        if (values(e, size, t, "tile tag") == DSX_OK) v = t[0];
        static const char* names[] = {"TileWidth", "TileLength", "TileOffsets", "TileByteCounts"};
        return fail(DSX_ERR_INVALID, "%s: tiled TIFF (%s = %llu) is not supported: strips only", path.c_str(),
                    names[e.tag - 322], (ull)v);
      }
      default: break;
    }
  }
  if (compression != 1)
    return fail(DSX_ERR_INVALID, "%s: Compression = %llu (%s) is not supported: uncompressed (1) only", path.c_str(),
                (ull)compression, compression_name(compression));
  if (pg.W < 1 || pg.H < 1 || pg.W > size || pg.H > size)
    return fail(DSX_ERR_INVALID, "%s: ImageWidth = %llu, ImageLength = %llu cannot be held by a file of %llu bytes",
                path.c_str(), (ull)pg.W, (ull)pg.H, (ull)size);
  if (pg.S < 1 || pg.S > 4)
    return fail(DSX_ERR_INVALID, "%s: SamplesPerPixel = %llu is not supported: 1..4", path.c_str(), (ull)pg.S);
  if (planar != 1 && pg.S > 1)
    return fail(DSX_ERR_INVALID, "%s: PlanarConfiguration = %llu (separate planes) is not supported: chunky (1) only",
                path.c_str(), (ull)planar);
  if (bits.empty()) bits.push_back(1);                     // the TIFF default: bilevel
  for (uint64_t b : bits)
    if (b != bits[0])
      return fail(DSX_ERR_INVALID, "%s: BitsPerSample differs between samples (%llu, %llu)", path.c_str(), (ull)bits[0], (ull)b);
  if (bits.size() != 1 && bits.size() != pg.S)
    return fail(DSX_ERR_INVALID, "%s: BitsPerSample has %llu values for SamplesPerPixel = %llu", path.c_str(),
                (ull)bits.size(), (ull)pg.S);
  pg.bits = bits[0];
  if (pg.bits != 8 && pg.bits != 16 && pg.bits != 32)
    return fail(DSX_ERR_INVALID, "%s: BitsPerSample = %llu is not supported: 8, 16, 32", path.c_str(), (ull)pg.bits);
  pg.format = format.empty() ? 1 : format[0];
  for (uint64_t v : format)
    if (v != pg.format) return fail(DSX_ERR_INVALID, "%s: SampleFormat differs between samples (%llu, %llu)", path.c_str(), (ull)pg.format, (ull)v);
  if (!(pg.format == 1 || (pg.format == 3 && pg.bits == 32)))
    return fail(DSX_ERR_INVALID, "%s: SampleFormat = %llu with BitsPerSample = %llu is not supported: unsigned integers of "
                "8 / 16 / 32 bits and 32-bit float", path.c_str(), (ull)pg.format, (ull)pg.bits);
  // strips
  uint64_t row, page;
  if (!mul_ok(pg.W, pg.S * (pg.bits / 8), row) || !mul_ok(row, pg.H, page) || page > size)
    return fail(DSX_ERR_INVALID, "%s: a page of %llu x %llu x %llu samples of %llu bits does not fit the file (%llu bytes): truncated or corrupt",
                path.c_str(), (ull)pg.H, (ull)pg.W, (ull)pg.S, (ull)pg.bits, (ull)size);
  if (rows_per_strip < 1) return fail(DSX_ERR_INVALID, "%s: RowsPerStrip = 0", path.c_str());
  const uint64_t rps = rows_per_strip < pg.H ? rows_per_strip : pg.H;
  const uint64_t n_strips = (pg.H + rps - 1) / rps;
  if (pg.off.size() != n_strips)
    return fail(DSX_ERR_INVALID, "%s: StripOffsets has %llu values, %llu rows in strips of %llu need %llu", path.c_str(),
                (ull)pg.off.size(), (ull)pg.H, (ull)rps, (ull)n_strips);
  if (has_counts && counts.size() != n_strips)
    return fail(DSX_ERR_INVALID, "%s: StripByteCounts has %llu values for %llu strips", path.c_str(), (ull)counts.size(), (ull)n_strips);
  pg.rows.resize((size_t)n_strips);
  for (uint64_t s = 0; s < n_strips; ++s) {
    const uint64_t r = s + 1 < n_strips ? rps : pg.H - s * rps;
    const uint64_t need = r * row;                         // <= page <= size
    pg.rows[(size_t)s] = r;
    if (has_counts && counts[(size_t)s] != need)
      return fail(DSX_ERR_INVALID, "%s: strip %llu holds %llu bytes, %llu rows of %llu bytes need %llu", path.c_str(), (ull)s,
                  (ull)counts[(size_t)s], (ull)r, (ull)row, (ull)need);
    if (!inside(pg.off[(size_t)s], need, size))
      return fail(DSX_ERR_INVALID, "%s: strip %llu at offset %llu (%llu bytes) lies outside the file (%llu bytes): truncated or corrupt",
                  path.c_str(), (ull)s, (ull)pg.off[(size_t)s], (ull)need, (ull)size);
  }
  return DSX_OK;
}

int dsx_tiff::parse() {
  unsigned char h[16];
  int rc = read_at(0, h, 8, "header");
  if (rc) return rc;
  if ((h[0] != 'I' && h[0] != 'M') || h[0] != h[1])
    return fail(DSX_ERR_INVALID, "%s: not a TIFF file (byte-order mark 0x%02x%02x)", path.c_str(), h[0], h[1]);
  swap = (h[0] == 'I') != host_le();
  const uint64_t magic = u(h + 2, 2);
  uint64_t at;
  if (magic == 42) { big = false; at = u(h + 4, 4); }
  else if (magic == 43) {
    big = true;
    if ((rc = read_at(0, h, 16, "BigTIFF header"))) return rc;
    if (u(h + 4, 2) != 8 || u(h + 6, 2) != 0)
      return fail(DSX_ERR_INVALID, "%s: BigTIFF header with offset size %llu", path.c_str(), (ull)u(h + 4, 2));
    at = u(h + 8, 8);
  } else return fail(DSX_ERR_INVALID, "%s: not a TIFF file (magic %llu, expected 42 or 43)", path.c_str(), (ull)magic);
  std::unordered_set<uint64_t> seen;
  while (at != 0) {
    if (!seen.insert(at).second) return fail(DSX_ERR_INVALID, "%s: the IFD chain loops back to offset %llu", path.c_str(), (ull)at);
    Page pg;
    uint64_t next = 0;
    if ((rc = parse_ifd(at, next, pg))) return rc;
    if (!pages.empty()) {
      const Page& a = pages[0];
      if (pg.W != a.W || pg.H != a.H || pg.S != a.S || pg.bits != a.bits || pg.format != a.format)
        return fail(DSX_ERR_INVALID, "%s: page %llu is %llu x %llu x %llu (%llu bits, SampleFormat %llu) but page 0 is "
                    "%llu x %llu x %llu (%llu bits, SampleFormat %llu): pages of differing shape or type are not supported",
                    path.c_str(), (ull)pages.size(), (ull)pg.H, (ull)pg.W, (ull)pg.S, (ull)pg.bits, (ull)pg.format,
                    (ull)a.H, (ull)a.W, (ull)a.S, (ull)a.bits, (ull)a.format);
      pg.description.clear();
    }
    pages.push_back(std::move(pg));
    at = next;
  }
  if (pages.empty()) return fail(DSX_ERR_INVALID, "%s: no image file directory", path.c_str());
  const Page& a = pages[0];
  dtype = a.format == 3 ? DSX_PIX_F32 : a.bits == 8 ? DSX_PIX_U8 : a.bits == 16 ? DSX_PIX_U16 : DSX_PIX_U32;
  sample_bytes = a.bits / 8;
  row_bytes = a.W * a.S * sample_bytes;
  page_bytes = row_bytes * a.H;
  n_pages = (int64_t)pages.size();
  // ImageJ's contiguous stack: one IFD, "images=N" planes back to back from the first strip
  if (pages.size() == 1 && a.description.compare(0, 7, "ImageJ=") == 0) {
    const size_t k = a.description.find("images=");
    uint64_t n = 0;
    if (k != std::string::npos)
      for (size_t i = k + 7; i < a.description.size() && a.description[i] >= '0' && a.description[i] <= '9' && n < (1ull << 40); ++i)
        n = n * 10 + (uint64_t)(a.description[i] - '0');
    bool packed = true;
    for (size_t s = 0; s + 1 < a.off.size(); ++s) packed = packed && a.off[s + 1] == a.off[s] + a.rows[s] * row_bytes;
    uint64_t total;
    if (n > 1 && packed && mul_ok(n, page_bytes, total) && inside(a.off[0], total, size)) {
      n_pages = (int64_t)n;
      contiguous = true;
    }
  }
  return DSX_OK;
}

extern "C" int dsx_tiff_open(const char* path, dsx_tiff** out) {
  if (!path || !out) return fail(DSX_ERR_INVALID, "dsx_tiff_open: null argument");
  *out = nullptr;
  dsx_tiff* t = new dsx_tiff();
  t->path = path;
  t->f = fopen(path, "rb");
  if (!t->f) { delete t; return fail(DSX_ERR_INVALID, "%s: cannot be opened", path); }
  if (fseeko(t->f, 0, SEEK_END) != 0 || ftello(t->f) < 0) { delete t; return fail(DSX_ERR_INVALID, "%s: cannot be sized", path); }
  t->size = (uint64_t)ftello(t->f);
  const int rc = t->parse();
  if (rc) { delete t; return rc; }
  *out = t;
  return DSX_OK;
}

extern "C" int dsx_tiff_info(const dsx_tiff* t, int64_t shape[4], int* dtype) {
  if (!t || !shape || !dtype) return fail(DSX_ERR_INVALID, "dsx_tiff_info: null argument");
  shape[0] = t->n_pages; shape[1] = (int64_t)t->pages[0].H; shape[2] = (int64_t)t->pages[0].W; shape[3] = (int64_t)t->pages[0].S;
  *dtype = t->dtype;
  return DSX_OK;
}

extern "C" int dsx_tiff_read(dsx_tiff* t, int64_t first_page, int64_t n_pages, void* dst, size_t capacity) {
  if (!t || !dst) return fail(DSX_ERR_INVALID, "dsx_tiff_read: null argument");
  if (first_page < 0 || n_pages < 1 || first_page > t->n_pages || n_pages > t->n_pages - first_page)
    return fail(DSX_ERR_INVALID, "%s: pages [%lld, %lld) asked of %lld", t->path.c_str(), (long long)first_page,
                (long long)(first_page + n_pages), (long long)t->n_pages);
  uint64_t total;
  if (!mul_ok((uint64_t)n_pages, t->page_bytes, total) || total > capacity)
    return fail(DSX_ERR_INVALID, "%s: %lld pages of %llu bytes do not fit the destination (%llu bytes)", t->path.c_str(),
                (long long)n_pages, (ull)t->page_bytes, (ull)capacity);
  unsigned char* d = (unsigned char*)dst;
  int rc;
  if (t->contiguous) {     // open checked that all planes lie inside the file
    if ((rc = t->read_at(t->pages[0].off[0] + (uint64_t)first_page * t->page_bytes, d, total, "ImageJ stack planes"))) return rc;
  } else {
    for (int64_t p = first_page; p < first_page + n_pages; ++p) {
      const Page& pg = t->pages[(size_t)p];
      for (size_t s = 0; s < pg.off.size(); ++s) {
        const uint64_t len = pg.rows[s] * t->row_bytes;
        if ((rc = t->read_at(pg.off[s], d, len, "strip"))) return rc;
        d += len;
      }
    }
  }
  if (t->swap && t->sample_bytes > 1) {
    unsigned char* q = (unsigned char*)dst;
    const uint64_t sb = t->sample_bytes;
    for (uint64_t i = 0; i < total; i += sb)
      for (uint64_t k = 0; k < sb / 2; ++k) { const unsigned char x = q[i + k]; q[i + k] = q[i + sb - 1 - k]; q[i + sb - 1 - k] = x; }
  }
  return DSX_OK;
}

extern "C" void dsx_tiff_close(dsx_tiff* t) { delete t; }

// ------------------------------------------------------------------ writer
namespace {
struct Out {
  FILE* f;
  bool ok = true;
  void bytes(const void* p, size_t n) { if (ok && n && fwrite(p, 1, n, f) != n) ok = false; }
  void le(uint64_t v, int n) { unsigned char b[8]; for (int i = 0; i < n; ++i) b[i] = (unsigned char)(v >> (8 * i)); bytes(b, (size_t)n); }
};
}  // namespace

extern "C" int dsx_tiff_write(const char* path, const void* data, int64_t pages, int64_t H, int64_t W, int dtype,
                              const char* description, int bigtiff) {
  if (!path || !data) return fail(DSX_ERR_INVALID, "dsx_tiff_write: null argument");
  if (pages < 1 || H < 1 || W < 1 || H > 0x7fffffff || W > 0x7fffffff || pages > (1ll << 40))
    return fail(DSX_ERR_INVALID, "dsx_tiff_write: %lld pages of %lld x %lld", (long long)pages, (long long)H, (long long)W);
  if (dtype != DSX_PIX_U8 && dtype != DSX_PIX_U16 && dtype != DSX_PIX_F32)
    return fail(DSX_ERR_INVALID, "dsx_tiff_write: pixel type %d is not written: uint8, uint16, float32", dtype);
  if (bigtiff < -1 || bigtiff > 1) return fail(DSX_ERR_INVALID, "dsx_tiff_write: bigtiff = %d (0, 1 or -1 for auto)", bigtiff);
  const uint64_t sb = dtype == DSX_PIX_U8 ? 1 : dtype == DSX_PIX_U16 ? 2 : 4;
  uint64_t page, total;
  if (!mul_ok((uint64_t)H * (uint64_t)W, sb, page) || !mul_ok(page, (uint64_t)pages, total) || total > (1ull << 62))
    return fail(DSX_ERR_INVALID, "dsx_tiff_write: the stack is too large");
  const uint64_t desc_len = description ? strlen(description) + 1 : 0;
  const unsigned n_first = description ? 11 : 10;
  // layout: header, the pixel data of all pages back to back, the description, the IFDs
  const uint64_t classic_end = 8 + total + desc_len + 1 + (uint64_t)pages * (2 + 12 * 11 + 4);
  const bool big = bigtiff == 1 || (bigtiff == -1 && classic_end > 0xffffffffull);
  if (!big && classic_end > 0xffffffffull)
    return fail(DSX_ERR_INVALID, "dsx_tiff_write: %llu bytes need BigTIFF (bigtiff = 1 or -1)", (ull)classic_end);
  const uint64_t hdr = big ? 16 : 8, ent = big ? 20 : 12, cnt = big ? 8 : 2, offb = big ? 8 : 4;
  const uint64_t data_at = hdr;
  const uint64_t desc_at = data_at + total;
  uint64_t ifd_at = desc_at + desc_len;
  const uint64_t pad = ifd_at & 1;
  ifd_at += pad;
  Out o{fopen(path, "wb")};
  if (!o.f) return fail(DSX_ERR_INVALID, "%s: cannot be created", path);
  o.bytes("II", 2);
  if (big) { o.le(43, 2); o.le(8, 2); o.le(0, 2); o.le(ifd_at, 8); }
  else { o.le(42, 2); o.le(ifd_at, 4); }
  const unsigned char* src = (const unsigned char*)data;
  for (uint64_t done = 0; done < total && o.ok;) {         // pieces of 256 MiB at most
    const uint64_t n = total - done < (1ull << 28) ? total - done : (1ull << 28);
    o.bytes(src + done, (size_t)n);
    done += n;
  }
  if (description) o.bytes(description, (size_t)desc_len);
  if (pad) o.le(0, 1);
  auto entry = [&](unsigned tag, unsigned type, uint64_t count, uint64_t value) {
    o.le(tag, 2); o.le(type, 2); o.le(count, big ? 8 : 4);
    const int vs = type == 3 ? 2 : type == 16 ? 8 : 4;     // SHORT, LONG8, else LONG / ASCII offset
    if (type == 2) o.le(value, (int)offb);
    else { o.le(value, vs); o.le(0, (int)offb - vs); }
  };
  const unsigned off_type = big ? 16 : 4;
  uint64_t at = ifd_at;
  for (int64_t p = 0; p < pages; ++p) {
    const unsigned n = p == 0 ? n_first : 10;
    const uint64_t next = p + 1 < pages ? at + cnt + n * ent + offb : 0;
    o.le(n, (int)cnt);
    entry(256, 4, 1, (uint64_t)W);
    entry(257, 4, 1, (uint64_t)H);
    entry(258, 3, 1, sb * 8);
    entry(259, 3, 1, 1);
    entry(262, 3, 1, 1);                                   // BlackIsZero
    if (p == 0 && description) {
      if (desc_len <= offb) {                              // short strings sit in the value field
        o.le(270, 2); o.le(2, 2); o.le(desc_len, big ? 8 : 4);
        unsigned char v[8] = {0};
        memcpy(v, description, (size_t)desc_len);
        o.bytes(v, (size_t)offb);
      } else entry(270, 2, desc_len, desc_at);
    }
    entry(273, off_type, 1, data_at + (uint64_t)p * page);
    entry(277, 3, 1, 1);
    entry(278, 4, 1, (uint64_t)H);
    entry(279, off_type, 1, page);
    entry(339, 3, 1, dtype == DSX_PIX_F32 ? 3 : 1);
    o.le(next, (int)offb);
    at = next;
  }
  const bool closed = fclose(o.f) == 0;
  if (!o.ok || !closed) return fail(DSX_ERR_INVALID, "%s: write failed (disk full?)", path);
  return DSX_OK;
}
