// tiff_san_main.cpp — stand-alone driver of the TIFF reader for sanitizer runs on the host (tools/tiff_sanitize.sh):
// open / info / read / close on every regular file of a directory.  A file may be refused (with a message); it may
// not crash, read out of bounds or return fewer bytes than it declares.  Exit status 0: every file was either read
// completely or refused with a non-empty message.
#include <dirent.h>
#include <sys/stat.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/dsx.h"

// the library's error state, which dsx_tiff.cpp expects from the rest of libdsx
static std::string g_err;
namespace dsx {
int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace dsx
extern "C" const char* dsx_last_error(void) { return g_err.c_str(); }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s DIRECTORY\n", argv[0]); return 2; }
  DIR* d = opendir(argv[1]);
  if (!d) { fprintf(stderr, "%s: cannot be listed\n", argv[1]); return 2; }
  long files = 0, read_ok = 0, refused = 0, bad = 0;
  while (dirent* e = readdir(d)) {
    const std::string path = std::string(argv[1]) + "/" + e->d_name;
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) continue;
    ++files;
    g_err.clear();
    dsx_tiff* h = nullptr;
    int rc = dsx_tiff_open(path.c_str(), &h);
    if (rc == DSX_OK) {
      int64_t shape[4];
      int dtype = -1;
      rc = dsx_tiff_info(h, shape, &dtype);
      if (rc == DSX_OK) {
        const size_t sample = dtype == DSX_PIX_U8 ? 1 : dtype == DSX_PIX_U16 ? 2 : 4;
        const size_t bytes = (size_t)shape[0] * (size_t)shape[1] * (size_t)shape[2] * (size_t)shape[3] * sample;
        std::vector<unsigned char> buf(bytes);   // exactly as large as declared: a longer read is a heap overflow
        rc = dsx_tiff_read(h, 0, shape[0], buf.data(), buf.size());
        if (rc == DSX_OK) {                      // the pages one at a time give the same bytes
          std::vector<unsigned char> one(bytes / (size_t)shape[0]);
          for (int64_t p = 0; p < shape[0] && rc == DSX_OK; ++p) {
            rc = dsx_tiff_read(h, p, 1, one.data(), one.size());
            if (rc == DSX_OK && memcmp(one.data(), buf.data() + (size_t)p * one.size(), one.size()) != 0) {
              fprintf(stderr, "%s: page %lld differs between the whole and the single read\n", path.c_str(), (long long)p);
              ++bad;
            }
          }
        }
      }
      dsx_tiff_close(h);
    }
    if (rc == DSX_OK) ++read_ok;
    else if (g_err.empty()) { fprintf(stderr, "%s: status %d without a message\n", path.c_str(), rc); ++bad; }
    else ++refused;
  }
  closedir(d);
  printf("%ld files: %ld read, %ld refused, %ld bad\n", files, read_ok, refused, bad);
  return bad == 0 && files > 0 ? 0 : 1;
}
