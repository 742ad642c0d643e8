// dsx_model.cpp — the UNet model: topology and parameter table in the reference's state_dict order, weight repacking
// into MFMA fragment order, the device image (finalize, packed export) and the flop count.  Also the library's error
// state.  C ABI in include/dsx.h.
#include "dsx_rt.h"

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
int dsx::fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

extern "C" const char* dsx_last_error(void) { return g_err.c_str(); }
extern "C" int dsx_abi_version(void) { return DSX_ABI_VERSION; }
extern "C" int dsx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

// ------------------------------------------------------------------ model
static int add_param(dsx_model* m, const std::string& name, std::initializer_list<int64_t> shape) {
  Param p;
  p.name = name;
  p.shape.assign(shape.begin(), shape.end());
  m->params.push_back(std::move(p));
  return (int)m->params.size() - 1;
}
static ConvW add_conv(dsx_model* m, const std::string& pfx, int cin, int cout, int ks, bool bias) {
  ConvW c;
  c.cin = cin; c.cout = cout; c.ks = ks;
  c.pw = add_param(m, pfx + ".weight", {cout, cin, ks, ks});
  if (bias) c.pb = add_param(m, pfx + ".bias", {cout});
  return c;
}
static GnW add_gn(dsx_model* m, const std::string& pfx, int C) {
  GnW g;
  g.C = C;
  g.pg = add_param(m, pfx + ".weight", {C});
  g.pb = add_param(m, pfx + ".bias", {C});
  return g;
}
static LinW add_lin(dsx_model* m, const std::string& pfx, int in, int out) {
  LinW l;
  l.in = in; l.out = out;
  l.pw = add_param(m, pfx + ".weight", {out, in});
  l.pb = add_param(m, pfx + ".bias", {out});
  return l;
}

// ResnetBlocWithAttn in state_dict order (sr3 unet.py:94-158, ddpm unet.py:78-146)
static void add_res(dsx_model* m, const std::string& pfx, Module& md) {
  const dsx_unet_cfg& c = m->cfg;
  const std::string rb = pfx + ".res_block";
  if (c.with_time_emb) {
    md.film = add_lin(m, c.flavour == DSX_FLAVOUR_SR3 ? rb + ".noise_func.noise_func.0" : rb + ".mlp.1",
                      c.inner_channel, md.cout);
    md.film_off = m->F;
    m->F += md.cout;
  }
  md.gn1 = add_gn(m, rb + ".block1.block.0", md.cin);
  md.conv1 = add_conv(m, rb + ".block1.block.3", md.cin, md.cout, 3, true);
  md.gn2 = add_gn(m, rb + ".block2.block.0", md.cout);
  md.conv2 = add_conv(m, rb + ".block2.block.3", md.cout, md.cout, 3, true);
  md.has_res = md.cin != md.cout;
  if (md.has_res) md.res = add_conv(m, rb + ".res_conv", md.cin, md.cout, 1, true);
  if (md.attn) {
    md.gna = add_gn(m, pfx + ".attn.norm", md.cout);
    md.qkv = add_conv(m, pfx + ".attn.qkv", md.cout, 3 * md.cout, 1, false);
    md.out = add_conv(m, pfx + ".attn.out", md.cout, md.cout, 1, true);
  }
}

extern "C" int dsx_model_create(const dsx_unet_cfg* cfg, dsx_model** out) {
  if (!cfg || !out) return fail(DSX_ERR_INVALID, "null argument");
  if (cfg->n_mults < 1 || cfg->n_mults > 8 || cfg->n_attn_res < 0 || cfg->n_attn_res > 8)
    return fail(DSX_ERR_INVALID, "bad n_mults/n_attn_res");
  if (cfg->inner_channel < 4 || cfg->inner_channel % 4 || cfg->norm_groups < 1)
    return fail(DSX_ERR_INVALID, "inner_channel must be a positive multiple of 4");
  for (int i = 0; i < cfg->n_mults; ++i)
    if ((cfg->inner_channel * cfg->channel_mults[i]) % cfg->norm_groups)
      return fail(DSX_ERR_INVALID, "norm_groups must divide every level's channel count");
  dsx_model* m = new dsx_model();
  m->cfg = *cfg;
  const int inner = cfg->inner_channel;
  auto in_attn = [&](int res) {
    for (int i = 0; i < cfg->n_attn_res; ++i)
      if (cfg->attn_res[i] == res) return true;
    return false;
  };
  // time embedding MLP (sr3 unet.py:177-187 / ddpm unet.py:163-173)
  if (cfg->with_time_emb) {
    if (cfg->flavour == DSX_FLAVOUR_SR3) {
      m->t1 = add_lin(m, "noise_level_mlp.1", inner, 4 * inner);
      m->t2 = add_lin(m, "noise_level_mlp.3", 4 * inner, inner);
    } else {
      m->p_invfreq = add_param(m, "time_mlp.0.inv_freq", {inner / 2});
      m->t1 = add_lin(m, "time_mlp.1", inner, 4 * inner);
      m->t2 = add_lin(m, "time_mlp.3", 4 * inner, inner);
    }
  }
  // downs
  int pre = inner, now_res = cfg->image_size, idx = 0;
  std::vector<int> feat{pre};
  {
    Module md{};
    md.kind = 0; md.section = 0; md.cin = cfg->in_channel; md.cout = inner;
    md.conv = add_conv(m, "downs.0", cfg->in_channel, inner, 3, true);
    m->mods.push_back(md);
    idx = 1;
  }
  for (int ind = 0; ind < cfg->n_mults; ++ind) {
    const bool last = ind == cfg->n_mults - 1;
    const bool use_attn = in_attn(now_res);
    const int ch = inner * cfg->channel_mults[ind];
    for (int r = 0; r < cfg->res_blocks; ++r) {
      Module md{};
      md.kind = 1; md.section = 0; md.cin = pre; md.cout = ch; md.attn = use_attn;
      add_res(m, "downs." + std::to_string(idx++), md);
      m->mods.push_back(md);
      feat.push_back(ch);
      pre = ch;
    }
    if (!last) {
      Module md{};
      md.kind = 2; md.section = 0; md.cin = pre; md.cout = pre;
      md.conv = add_conv(m, "downs." + std::to_string(idx++) + ".conv", pre, pre, 3, true);
      m->mods.push_back(md);
      feat.push_back(pre);
      now_res /= 2;
    }
  }
  for (int k = 0; k < 2; ++k) {
    Module md{};
    md.kind = 1; md.section = 1; md.cin = pre; md.cout = pre; md.attn = (k == 0);
    add_res(m, "mid." + std::to_string(k), md);
    m->mods.push_back(md);
  }
  idx = 0;
  for (int ind = cfg->n_mults - 1; ind >= 0; --ind) {
    const bool last = ind < 1;
    const bool use_attn = in_attn(now_res);
    const int ch = inner * cfg->channel_mults[ind];
    for (int r = 0; r < cfg->res_blocks + 1; ++r) {
      Module md{};
      md.kind = 1; md.section = 2; md.skip = feat.back(); feat.pop_back();
      md.cin = pre + md.skip; md.cout = ch; md.attn = use_attn;
      if (md.cin % cfg->norm_groups) {
        delete m;
        return fail(DSX_ERR_INVALID, "norm_groups must divide concatenated channel counts");
      }
      add_res(m, "ups." + std::to_string(idx++), md);
      m->mods.push_back(md);
      pre = ch;
    }
    if (!last) {
      Module md{};
      md.kind = 3; md.section = 2; md.cin = pre; md.cout = pre;
      md.conv = add_conv(m, "ups." + std::to_string(idx++) + ".conv", pre, pre, 3, true);
      m->mods.push_back(md);
      now_res *= 2;
    }
  }
  {
    Module md{};
    md.kind = 4; md.section = 3; md.cin = pre;
    md.cout = cfg->out_channel > 0 ? cfg->out_channel : cfg->in_channel;
    md.gn1 = add_gn(m, "final_conv.block.0", pre);
    md.conv = add_conv(m, "final_conv.block.3", pre, md.cout, 3, true);
    m->mods.push_back(md);
  }
  m->want_naive = read_plan_knobs().conv_naive;
  *out = m;
  return DSX_OK;
}

extern "C" void dsx_model_destroy(dsx_model* m) { delete m; }
extern "C" int dsx_model_num_params(const dsx_model* m) { return m ? (int)m->params.size() : 0; }
extern "C" int dsx_model_param_info(const dsx_model* m, int i, char* name, int cap, int* ndim,
                                    int64_t shape[4]) {
  if (!m || i < 0 || i >= (int)m->params.size()) return fail(DSX_ERR_INVALID, "bad param index");
  const Param& p = m->params[i];
  if (name && cap > 0) snprintf(name, cap, "%s", p.name.c_str());
  if (ndim) *ndim = (int)p.shape.size();
  if (shape)
    for (size_t k = 0; k < 4; ++k) shape[k] = k < p.shape.size() ? p.shape[k] : 1;
  return DSX_OK;
}
extern "C" int dsx_model_set_param(dsx_model* m, int i, const float* data, int64_t numel) {
  if (!m || !data || i < 0 || i >= (int)m->params.size()) return fail(DSX_ERR_INVALID, "bad argument");
  Param& p = m->params[i];
  if (numel != p.numel())
    return fail(DSX_ERR_INVALID, "param %s: got %lld elements, expected %lld", p.name.c_str(),
                (long long)numel, (long long)p.numel());
  p.host.assign(data, data + numel);
  p.set = true;
  m->finalized = false;
  return DSX_OK;
}
extern "C" int dsx_model_set_posenc_freq(dsx_model* m, const float* f, int count) {
  if (!m || !f || count != m->cfg.inner_channel / 2) return fail(DSX_ERR_INVALID, "bad freq table");
  m->freq.assign(f, f + count);
  m->freq_set = true;
  m->finalized = false;
  return DSX_OK;
}

// fp32 -> bf16 round-to-nearest-even (finite inputs)
static inline uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// packed geometry of one conv: 64-byte input-channel chunks (padded to the staging group) and 32-channel N blocks
void dsx::conv_geometry(int cout, int cin, int ks, int dtype, int& kchunks, int& nblocks) {
  const int KC = dtype != DSX_DTYPE_F32 ? 32 : 16;
  const int mult = conv_chunk_multiple(ks);
  kchunks = ((cin + KC - 1) / KC + mult - 1) / mult * mult;
  nblocks = (cout + 31) / 32;
}

// fp32 -> fp16 round-to-nearest-even
static inline uint16_t f2h(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}

// OIHW fp32 -> [nblk][kchunk][tap][half][lane][16 B] (see dsx_conv_mfma.hip header)
static void pack_conv(const float* w, int cout, int cin, int ks, int dtype, std::vector<char>& dst,
                      int& kchunks, int& nblocks) {
  const int KC = dtype != DSX_DTYPE_F32 ? 32 : 16, EPL = dtype != DSX_DTYPE_F32 ? 8 : 4, taps = ks * ks;
  conv_geometry(cout, cin, ks, dtype, kchunks, nblocks);
  dst.assign((size_t)nblocks * kchunks * taps * 2 * 64 * 16, 0);
  for (int nb = 0; nb < nblocks; ++nb)
    for (int kc = 0; kc < kchunks; ++kc)
      for (int tap = 0; tap < taps; ++tap)
        for (int fs = 0; fs < 2; ++fs)
          for (int lane = 0; lane < 64; ++lane) {
            // MFMA A row i = q + 8*j + 4*hh carries output channel 16*hh + 4*j + q of the block, so that a
            // lane's 16 accumulator registers are 16 consecutive channels (dsx_conv_common.h, store16)
            const int i = lane & 31, h = lane >> 5;
            const int n = nb * 32 + 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3);
            char* p = dst.data() + ((((size_t)(nb * kchunks + kc) * taps + tap) * 2 + fs) * 64 + lane) * 16;
            for (int j = 0; j < EPL; ++j) {
              const int c = kc * KC + (KC / 2) * fs + EPL * h + j;
              float v = 0.f;
              if (n < cout && c < cin) v = w[((size_t)n * cin + c) * taps + tap];
              if (dtype == DSX_DTYPE_BF16) { uint16_t b = f2bf(v); memcpy(p + 2 * j, &b, 2); }
              else if (dtype == DSX_DTYPE_F16) { uint16_t b = f2h(v); memcpy(p + 2 * j, &b, 2); }
              else memcpy(p + 4 * j, &v, 4);
            }
          }
}

// OIHW fp32 3x3 weights with cin <= 7 -> k_conv_first's operand: K = 9 cin as one dimension, k = tap * cin + c.
// 16-bit: [nblk][4 k-steps][lane][8 elements], element j of lane (i, h) = W[n(i)][16 s + 8 h + j];
// fp32: [nblk][32 k-steps][lane] floats, lane (i, h) = W[n(i)][2 s + h].  Rows permuted like pack_conv.
static void pack_first(const float* w, int cout, int cin, int dtype, std::vector<char>& dst) {
  const int K = 9 * cin, nblocks = (cout + 31) / 32;
  auto wk = [&](int n, int k) -> float {
    if (n >= cout || k >= K) return 0.f;
    const int tap = k / cin, c = k % cin;
    return w[((size_t)n * cin + c) * 9 + tap];
  };
  auto row = [](int nb, int i) { return nb * 32 + 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3); };
  if (dtype == DSX_DTYPE_F32) {
    dst.assign((size_t)nblocks * 32 * 64 * 4, 0);
    for (int nb = 0; nb < nblocks; ++nb)
      for (int s = 0; s < 32; ++s)
        for (int lane = 0; lane < 64; ++lane) {
          const float v = wk(row(nb, lane & 31), 2 * s + (lane >> 5));
          memcpy(dst.data() + (((size_t)nb * 32 + s) * 64 + lane) * 4, &v, 4);
        }
  } else {
    dst.assign((size_t)nblocks * 4 * 64 * 16, 0);
    for (int nb = 0; nb < nblocks; ++nb)
      for (int s = 0; s < 4; ++s)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const float v = wk(row(nb, lane & 31), 16 * s + 8 * (lane >> 5) + j);
            const uint16_t hbits = dtype == DSX_DTYPE_BF16 ? f2bf(v) : f2h(v);
            memcpy(dst.data() + ((((size_t)nb * 4 + s) * 64 + lane) * 8 + j) * 2, &hbits, 2);
          }
  }
}

namespace {
// One host image of everything the model keeps on the device (fragment-ordered conv weights, biases, GroupNorm
// affine parameters, time-embedding MLP, stacked FiLM linears).  With `write` false only the layout is computed
// (offsets and the total size): dsx_model_finalize_packed uploads a cached image into exactly this layout.
struct DevImage {
  bool write;
  std::vector<char> buf;
  size_t size = 0;
  struct Fix { void** dst; size_t off; };
  std::vector<Fix> fix;
  size_t reserve(size_t bytes) {
    const size_t off = (size + 255) & ~(size_t)255;
    size = off + bytes;
    if (write) buf.resize(size);
    return off;
  }
  void put(const void* src, size_t bytes, void** dst) {
    const size_t off = reserve(bytes);
    if (write) memcpy(buf.data() + off, src, bytes);
    fix.push_back({dst, off});
  }
};
}  // namespace

// layout (and, with img.write, contents) of the device image for `dtype`; the conv geometry is stored in the model
static int build_image(dsx_model* m, int dtype, DevImage& img) {
  const int inner = m->cfg.inner_channel;
  if (img.write) {
    for (int i = 0; i < (int)m->params.size(); ++i) {
      if (m->params[i].set || i == m->p_invfreq) continue;  // inv_freq is derived below if absent
      return fail(DSX_ERR_MISSING, "parameter %s was never set", m->params[i].name.c_str());
    }
    if (m->cfg.with_time_emb) {
      if (m->cfg.flavour == DSX_FLAVOUR_DDPM) {
        Param& p = m->params[m->p_invfreq];
        if (p.set) m->freq = p.host;
        else {  // ddpm unet.py:22-26
          m->freq.resize(inner / 2);
          for (int k = 0; k < inner / 2; ++k) m->freq[k] = expf((float)(2 * k) * (float)(-log(10000.0) / inner));
        }
      } else if (!m->freq_set) {  // sr3 unet.py:24-28
        m->freq.resize(inner / 2);
        for (int k = 0; k < inner / 2; ++k)
          m->freq[k] = expf((float)(-log(1e4)) * ((float)k / (float)(inner / 2)));
      }
    }
  }
  auto put_param = [&](int pi, float** dst) {   // one fp32 parameter as it is
    img.put(img.write ? m->params[pi].host.data() : nullptr, (size_t)m->params[pi].numel() * 4, (void**)dst);
  };
  auto put_conv = [&](ConvW& c) {
    if (c.pw < 0) return;
    conv_geometry(c.cout, c.cin, c.ks, dtype, c.kchunks, c.nblocks);
    std::vector<char> pk;
    size_t bytes = (size_t)c.nblocks * c.kchunks * c.ks * c.ks * 2 * 64 * 16;
    if (img.write) { pack_conv(m->params[c.pw].host.data(), c.cout, c.cin, c.ks, dtype, pk, c.kchunks, c.nblocks); bytes = pk.size(); }
    img.put(pk.data(), bytes, &c.pack);
    if (c.ks == 3 && c.cin <= 7) {
      std::vector<char> pf;
      size_t fb = (size_t)((c.cout + 31) / 32) * (dtype == DSX_DTYPE_F32 ? 32 * 64 * 4 : 4 * 64 * 16);
      if (img.write) { pack_first(m->params[c.pw].host.data(), c.cout, c.cin, dtype, pf); fb = pf.size(); }
      img.put(pf.data(), fb, &c.pack_first);
    }
    if (c.pb >= 0) put_param(c.pb, &c.bias);
    if (m->want_naive) {
      std::vector<float> nv;
      if (img.write) {
        nv.resize((size_t)c.cout * c.ks * c.ks * c.cin);
        const float* w = m->params[c.pw].host.data();
        for (int n = 0; n < c.cout; ++n)
          for (int ci = 0; ci < c.cin; ++ci)
            for (int t = 0; t < c.ks * c.ks; ++t)
              nv[((size_t)n * c.ks * c.ks + t) * c.cin + ci] = w[((size_t)n * c.cin + ci) * c.ks * c.ks + t];
      }
      img.put(nv.data(), (size_t)c.cout * c.ks * c.ks * c.cin * 4, (void**)&c.naive);
    }
  };
  auto put_gn = [&](GnW& g) {
    if (g.pg < 0) return;
    put_param(g.pg, &g.gamma);
    put_param(g.pb, &g.beta);
  };
  std::vector<float> wf, bf;
  if (img.write) { wf.resize((size_t)m->F * inner); bf.resize(m->F); }
  for (auto& md : m->mods) {
    put_conv(md.conv);
    put_gn(md.gn1); put_gn(md.gn2); put_gn(md.gna);
    put_conv(md.conv1); put_conv(md.conv2);
    if (md.has_res) put_conv(md.res);
    if (md.attn) { put_conv(md.qkv); put_conv(md.out); }
    if (md.film_off >= 0 && img.write) {
      memcpy(wf.data() + (size_t)md.film_off * inner, m->params[md.film.pw].host.data(),
             (size_t)md.cout * inner * 4);
      memcpy(bf.data() + md.film_off, m->params[md.film.pb].host.data(), (size_t)md.cout * 4);
      // the FiLM vector is only ever added to conv1's output: carry conv1's bias in it (one per-channel addend
      // in the conv epilogue instead of two; plan_res passes no bias for that conv)
      if (md.conv1.pb >= 0)
        for (int n = 0; n < md.cout; ++n) bf[md.film_off + n] += m->params[md.conv1.pb].host[n];
    }
  }
  if (m->cfg.with_time_emb) {
    img.put(m->freq.data(), (size_t)(inner / 2) * 4, (void**)&m->d_freq);
    put_param(m->t1.pw, &m->d_w1);
    put_param(m->t1.pb, &m->d_b1);
    put_param(m->t2.pw, &m->d_w2);
    put_param(m->t2.pb, &m->d_b2);
    img.put(wf.data(), (size_t)m->F * inner * 4, (void**)&m->d_wf);
    img.put(bf.data(), (size_t)m->F * 4, (void**)&m->d_bf);
  }
  return DSX_OK;
}

static int upload_image(dsx_model* m, int dtype, const DevImage& img, const void* bytes) {
  HIP_TRY(m->arena.upload(bytes, img.size));
  m->arena_bytes = img.size;
  for (auto& f : img.fix) *f.dst = m->arena.as<char>() + f.off;
  m->dtype = dtype;
  m->finalized = true;
  return DSX_OK;
}

static bool dtype_ok(int dtype) { return dtype == DSX_DTYPE_F32 || dtype == DSX_DTYPE_BF16 || dtype == DSX_DTYPE_F16; }

extern "C" int dsx_model_finalize(dsx_model* m, int dtype) {
  if (!m) return fail(DSX_ERR_INVALID, "null model");
  if (!dtype_ok(dtype)) return fail(DSX_ERR_INVALID, "bad dtype");
  DevImage img;
  img.write = true;
  int rc = build_image(m, dtype, img);
  if (rc) return rc;
  return upload_image(m, dtype, img, img.buf.data());
}

// ---- packed-weight cache (the one-time repack of a *_gen.pth, model/model.py:153-166): export the device image of a
// finalized model, and finalize a fresh model straight from such an image (no parameters set, no repacking)
extern "C" int dsx_model_packed_bytes(dsx_model* m, int dtype, size_t* bytes) {
  if (!m || !bytes || !dtype_ok(dtype)) return fail(DSX_ERR_INVALID, "bad argument");
  DevImage img;
  img.write = false;
  int rc = build_image(m, dtype, img);
  if (rc) return rc;
  *bytes = img.size;
  return DSX_OK;
}
extern "C" int dsx_model_export_packed(const dsx_model* m, void* host_buf, size_t capacity) {
  if (!m || !host_buf) return fail(DSX_ERR_INVALID, "null argument");
  if (!m->finalized) return fail(DSX_ERR_STATE, "finalize the model before exporting its packed image");
  if (capacity < m->arena_bytes) return fail(DSX_ERR_INVALID, "buffer of %zu bytes < %zu", capacity, m->arena_bytes);
  HIP_TRY(hipMemcpy(host_buf, m->arena.p, m->arena_bytes, hipMemcpyDeviceToHost));
  return DSX_OK;
}
extern "C" int dsx_model_finalize_packed(dsx_model* m, int dtype, const void* host_img, size_t bytes) {
  if (!m || !host_img || !dtype_ok(dtype)) return fail(DSX_ERR_INVALID, "bad argument");
  DevImage img;
  img.write = false;
  int rc = build_image(m, dtype, img);
  if (rc) return rc;
  if (img.size != bytes)
    return fail(DSX_ERR_INVALID, "packed image of %zu bytes does not fit this model / dtype (%zu expected)", bytes, img.size);
  return upload_image(m, dtype, img, host_img);
}

extern "C" double dsx_model_flops(const dsx_model* m, int H, int W) {
  if (!m) return 0;
  double fl = 0;
  int h = H, w = W;
  const int inner = m->cfg.inner_channel;
  auto conv = [&](const ConvW& c, int hh, int ww) {
    if (c.pw >= 0) fl += 2.0 * hh * ww * (double)c.cout * c.cin * c.ks * c.ks;
  };
  if (m->cfg.with_time_emb) fl += 2.0 * (inner * 4.0 * inner) * 2;
  for (auto& md : m->mods) {
    if (md.kind == 0) conv(md.conv, h, w);
    else if (md.kind == 2) { h /= 2; w /= 2; conv(md.conv, h, w); }
    else if (md.kind == 3) { h *= 2; w *= 2; conv(md.conv, h, w); }
    else if (md.kind == 4) conv(md.conv, h, w);
    else {
      conv(md.conv1, h, w); conv(md.conv2, h, w);
      if (md.has_res) conv(md.res, h, w);
      if (md.film_off >= 0) fl += 2.0 * inner * md.cout;
      if (md.attn) {
        conv(md.qkv, h, w); conv(md.out, h, w);
        const double L = (double)h * w;
        fl += 2.0 * 2.0 * L * L * md.cout;
      }
    }
  }
  return fl;
}
