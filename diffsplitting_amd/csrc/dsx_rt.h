// dsx_rt.h — what the host translation units of libdsx.so share (dsx_model.cpp, dsx_plan.cpp, dsx_exec.cpp,
// dsx_tiles.cpp, dsx_eval.cpp): the error state, the owners of HIP resources, the model and the executor with the
// plain-data types they contain, and the few functions called across files.  Internal; the public ABI is include/dsx.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dsx.h"
#include "dsx_kernels.h"

// The types below are seen by several translation units, so they live in the named namespace of dsx_kernels.h (a member
// of an anonymous namespace inside dsx_exec would give every file a dsx_exec of its own).
using namespace dsx;

namespace dsx {

// ------------------------------------------------------------------ errors
// records the message dsx_last_error returns (one per thread, dsx_model.cpp) and returns `code`
int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e__ = (expr);                                                              \
    if (e__ != hipSuccess)                                                                \
      return fail(DSX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),    \
                  __FILE__, __LINE__);                                                    \
  } while (0)

// ------------------------------------------------------------------ owners of HIP resources
// Move-only; each releases in its destructor and in reset().
struct DevBuf {            // device memory
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }   // `o` releases what this held
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }   // hipFree waits for launches that still use the buffer
  template <class T> T* as() const { return (T*)p; }
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  hipError_t upload(const void* host, size_t bytes) {
    const hipError_t e = alloc(bytes);
    return e != hipSuccess ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
  }
};
struct PinnedBuf {         // pinned host memory
  void* p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p, o.p); return *this; }
  ~PinnedBuf() { reset(); }
  void reset() { if (p) (void)hipHostFree(p); p = nullptr; }
  template <class T> T* as() const { return (T*)p; }
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
  ~Event() { reset(); }
  void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
  hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&e, flags); }
};
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
  ~Stream() { reset(); }
  void reset() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
  hipError_t create(unsigned flags) { reset(); return hipStreamCreateWithFlags(&s, flags); }
};
struct Graph {             // a captured graph and its executable instance (either may be missing)
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  Graph() = default;
  Graph(Graph&& o) noexcept : graph(o.graph), exec(o.exec) { o.graph = nullptr; o.exec = nullptr; }
  Graph& operator=(Graph&& o) noexcept { std::swap(graph, o.graph); std::swap(exec, o.exec); return *this; }
  ~Graph() { reset(); }
  void reset() {           // the caller has waited for the launches of `exec`
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr; graph = nullptr;
  }
};

// ------------------------------------------------------------------ planner knobs
// Every tuning switch of the launch planner, read from the environment by read_plan_knobs()
// once per plan: dsx_exec_create and dsx_plan_dry_run.  The defaults are the shipped plan.
struct PlanKnobs {
  bool conv_naive = false;   // DSX_CONV_IMPL=naive: the plain direct-conv kernel for every conv (cross-checks)
  int first = 1;             // DSX_FIRST: the UNet's first conv (few input channels) on the im2col-in-K kernel
  int img = 1;               // DSX_IMG: 8 x 8 maps on the image-resident kernel
  // warp-specialised persistent kernel (k_conv_ws): only needs ~one workgroup per CU
  int ws = 1;                // DSX_WS
  int ws_1x1 = 1;            // DSX_WS_1X1: 1 x 1 convs on it too
  int ws_min_grid = 224;     // DSX_WS_MIN_GRID: work items it needs (the parity tests lower it to force it onto small grids)
  // Two 64-byte chunks per (tile, group) item where the geometry allows it: under the 16 x 16 MFMA shape the loaders,
  // not the MFMAs, bound an item (their VALU stream gets 8 of every 16 issue cycles), and their per-item costs (DMA
  // issue, wait, fetch, barrier: ~1.3 k of 3.2 k cycles per 32 channels on the 64-pixel tile) are paid once per 64
  // channels this way.  Measured (same-box A/B): the 512-channel 16 x 16 layers -8 .. -11 %, a 256 -> 512 layer
  // with only 4 two-chunk groups +7 % (hence the 12-chunk minimum there); the 128 x 128 tile -2.6 % over its 22 launches.
  int ws_g2 = 1;             // DSX_WS_G2: several chunks per item for the 3 x 3 convs
  int ws_g2_min64 = 12;      // DSX_WS_G2_MIN64: chunks (64-pixel tile); fewer -> one-chunk groups
  int ws_g2_min128 = 4;      // DSX_WS_G2_MIN128: chunks (128-pixel tiles)
  int ws_g4_min64 = 16;      // DSX_WS_G4_MIN64: four chunks per item (64-pixel tile) from this many chunks
  int ws_c4 = 1;             // DSX_WS_C4: 1 x 1 convs, four chunks (128 input channels) per item
  int ws_c4_min = 8;         // DSX_WS_C4_MIN: chunks: at least two groups
  int ws_direct = 1;         // DSX_WS_DIRECT: plain 1 x 1 convs (no GroupNorm / Swish in front) on the direct rows: LDS-DMA
                             // straight into the MFMA images (ConvArgs::ws_direct); 0: the raw ring and the copying loaders
  // 1 x 1 convs with several N tiles: an XCD takes every N tile of its M tiles (ws_map 3).  With the N tiles dealt over
  // the XCDs (the 3 x 3 choice: there the weights are the larger operand) every L2 fetched most of the input: 65.7 MB
  // per launch of the 512 -> 1536 qkv conv against 18.4 MB algorithmic (PMC, profiles/r03_pmc_summary.txt).
  int ws_map3 = 1;           // DSX_WS_MAP3
  int xcd_bands = 1;         // DSX_XCD_BANDS: contiguous tile bands per XCD instead of round-robin tiles
  int host_fin = 1;          // DSX_HOST_FIN: residual 1 x 1 convs host the finalize of their block's second GroupNorm
  int prefetch = 1;          // DSX_PREFETCH: L2 weight prefetch (l2_prefetch in dsx_kernels.h)
  int prefetch_ws = 1;       // DSX_PREFETCH_WS: ... also carried by the previous k_conv_ws launch
  int fuse_stats = 1;        // DSX_FUSE_STATS: GroupNorm statistics in the conv (or split-K reduce) epilogue
  // Narrow outputs (<= 32 channels: the UNet's final conv, 64 -> 3 at full resolution): HBM-bound layers that the
  // generic 128 x 32 tile walked as two 32-channel groups with a barrier pair each and a 16 x 8 pixel halo.  The
  // two-chunk variant stages ALL input channels of a 16 x 16 (or 16 x 8) pixel patch once -- one load phase, one
  // conversion, one barrier, 36 MFMA steps per row block -- with three workgroups per CU overlapping their phases.
  int narrow_g2 = 1;         // DSX_NARROW_G2
  int min_grid = 512;        // DSX_MIN_GRID: workgroups a k_conv_mfma launch needs before split-K is considered
  int splitk = 1;            // DSX_SPLITK
  int attn_cs = 2;           // DSX_ATTN_CS: 2 = two attention workgroups per query tile on few-tile launches, 1 = one
  int stamp_op = -1;         // DSX_STAMP_OP=<conv ordinal>[,<block>]: in-kernel phase stamps of that launch (-DDSX_STAMPS)
  int stamp_block = 0;
  std::string plan_dump;     // DSX_PLAN_DUMP=<path>: every planning pass writes its launches there (dump_plan); empty = off
  int ablate = 0;            // DSX_ABLATE (-DDSX_DIAG builds only): timing experiments, results are wrong when non-zero
  // tile preference lists (TILE_* indices, "0,2,3,4"): the first that fills the chip wins
  std::vector<int> tiles_wide{TILE_128x128, TILE_64x128, TILE_64x64};              // DSX_TILES_WIDE
  std::vector<int> tiles_narrow{TILE_64x64, TILE_128x64};                          // DSX_TILES_NARROW
  std::vector<int> tiles_slim{TILE_128x32, TILE_64x64, TILE_128x64};               // DSX_TILES_SLIM: Cout <= 32
  std::vector<int> tiles_wide_split{TILE_64x128, TILE_128x128, TILE_64x64};        // DSX_TILES_WIDE_SPLIT
  std::vector<int> tiles_narrow_split{TILE_64x64, TILE_128x64};                    // DSX_TILES_NARROW_SPLIT
  std::vector<int> tiles_narrow_g2{TILE_256x32, TILE_128x32};                      // DSX_TILES_NARROW_G2
  // the 128 x 128 tile (2 x 2 waves of 64 pixels x 64 channels: each LDS pixel fragment feeds two MFMAs and each
  // converted group twice the MFMA work of the 64 x 128 tile) wherever it still fills the chip
  std::vector<int> tiles_ws_wide{TILE_128x128, TILE_64x128};                       // DSX_TILES_WS_WIDE
  std::vector<int> tiles_ws_wide_1x1{TILE_128x128, TILE_64x128};                   // DSX_TILES_WS_WIDE_1X1
  // 1 x 1 without GroupNorm / Swish in front (residual and attention-output convs): the loaders only copy, the kernel is
  // bound by the weight stream, and only the one-N-block tiles have the deep weight ring (measured: 32^2 layers -2 us each)
  std::vector<int> tiles_ws_wide_1x1_raw{TILE_64x128, TILE_128x128};               // DSX_TILES_WS_WIDE_1X1_RAW
  std::vector<int> tiles_ws_narrow{TILE_256x64, TILE_128x64, TILE_64x64};          // DSX_TILES_WS_NARROW
};

// ------------------------------------------------------------------ model
struct Param {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> host;
  bool set = false;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

struct ConvW {
  int pw = -1, pb = -1;  // param indices (weight, bias)
  int cin = 0, cout = 0, ks = 1;
  int kchunks = 0, nblocks = 0;
  void* pack = nullptr;     // device, fragment order
  void* pack_first = nullptr;   // device, im2col order of k_conv_first (few-input-channel 3x3 convs only)
  float* bias = nullptr;    // device
  float* naive = nullptr;   // device [Cout][ks][ks][Cin] (debug / 7x7 only)
};
struct GnW {
  int pg = -1, pb = -1;
  int C = 0;
  float* gamma = nullptr;
  float* beta = nullptr;
};
struct LinW {
  int pw = -1, pb = -1;
  int in = 0, out = 0;
};

struct Module {
  int kind;  // 0 conv_in, 1 res, 2 down, 3 up, 4 final
  int section;  // 0 downs, 1 mid, 2 ups, 3 final
  int cin = 0, cout = 0, skip = 0;
  bool attn = false;
  ConvW conv;             // conv_in / down / up / final conv
  GnW gn1, gn2, gna;      // res: block1/2 norms, attention norm; final: gn1
  ConvW conv1, conv2, res, qkv, out;
  bool has_res = false;
  LinW film;
  int film_off = -1;
};

}  // namespace dsx

struct dsx_model {
  dsx_unet_cfg cfg;
  std::vector<Param> params;
  std::vector<Module> mods;
  // time embedding
  int p_invfreq = -1;
  LinW t1, t2;
  std::vector<float> freq;  // inner/2
  bool freq_set = false;
  int F = 0;                // stacked FiLM outputs
  // device
  bool finalized = false;
  int dtype = 0;
  DevBuf arena;              // the device image (every device pointer of the model points into it)
  size_t arena_bytes = 0;
  float *d_freq = nullptr, *d_w1 = nullptr, *d_b1 = nullptr, *d_w2 = nullptr, *d_b2 = nullptr;
  float *d_wf = nullptr, *d_bf = nullptr;
  bool want_naive = false;  // DSX_CONV_IMPL=naive at creation: the device image also holds the naive kernel's weights
};

// ------------------------------------------------------------------ executor
namespace dsx {

struct Tensor {
  void* p = nullptr;       // NHWC in the storage type `st`
  int C = 0, H = 0, W = 0;
  int id = -1;             // index into dsx_exec::stats (copies of a Tensor share it)
  int st = 0;              // storage kind: 0 fp32, 1 bf16, 2 fp16 (DSX_DTYPE_*)
  int esz() const { return st ? 2 : 4; }
  char* at(size_t elem) const { return (char*)p + elem * esz(); }
};
struct StatInfo {          // GroupNorm partial sums of one tensor, produced at most once
  void* part = nullptr;    // double [B][nchunk][C][2] (k_chan_stats) or float (fused into the conv epilogue)
  int nchunk = 0;
  bool planned = false;
  bool f32 = false;
  StatPivot piv{nullptr, nullptr, 0};   // fp32 partials shifted by this pivot (k_conv_first, split-K reduce)
};

// One launch of the plan as plain data: what it computes (for profiling / roofline), which launch_* function takes
// it and every argument of that call.  launch_op() is the only place that turns one into a launch.
enum Launcher { L_CONV_FIRST, L_CONV_IMG, L_CONV_WS, L_CONV_MFMA, L_SPLITK_REDUCE, L_CONV_NAIVE, L_CHAN_STATS,
                L_GN_FINALIZE, L_ATTN };
struct ChanStatsArgs { const void* x; int xbf, B, HW, C, nchunk; double* part; };   // the parameters of launch_chan_stats
struct PlanOp {
  int kind = 0;            // DSX_OP_*
  std::string desc;
  double flops = 0;        // algorithmic 2*MAC
  double bytes = 0;        // algorithmic HBM bytes: inputs + outputs + weights, each once
  Launcher launcher = L_CONV_MFMA;
  int dtype = 0, tile = 0, ks = 0, stride = 0, col_split = 0;   // scalar launch parameters (a launcher reads the ones it takes)
  union Args {             // the member `launcher` names
    ConvArgs conv; SplitKReduceArgs reduce; NaiveConvArgs naive; ChanStatsArgs stats; GnFinArgs fin; AttnArgs attn;
    Args() { memset((void*)this, 0, sizeof *this); }
  } args;
};

}  // namespace dsx

struct dsx_exec {
  dsx_model* m = nullptr;
  PlanKnobs knobs;             // read when the plan is built
  int B = 0, H = 0, W = 0, cond_c = 0, x_c = 0;
  DevBuf ws_mem;               // the activation workspace, when this executor allocated one
  char* ws = nullptr;          // its base, borrowed: ws_mem.p, or the fake address of dsx_plan_dry_run (never freed)
  size_t ws_bytes = 0, ws_used = 0;
  bool sizing = true;
  std::vector<PlanOp> ops;     // the UNet forward (recorded by the planning pass only)
  int conv_ordinal = 0;
  // Late binding is a write into an earlier element of `ops` (-1: none).  L2 weight prefetch (l2_prefetch in
  // dsx_kernels.h): the previous image-resident conv and the previous k_conv_ws launch receive the weight slices of a
  // later conv once its kernel and tiling are known.  GroupNorm finalize hosted by the residual 1 x 1 conv in front of it
  // (k_conv_ws loader waves): `fin_host_op` is that conv, the next finalize planned writes its arguments there.
  int prev_img_op = -1, prev_ws_op = -1, fin_host_op = -1;
  bool fin_host_armed = false;   // both passes (launch count): the next finalize is hosted, it is no launch of its own
  unsigned long long* stamp_buf = nullptr;
  std::vector<StatInfo> stats;
  // fixed buffers
  Tensor in_cond, in_x, out;   // NHWC
  float* x_state = nullptr;    // sampler state, NHWC fp32 (== in_x.p unless activations are stored in bf16)
  float* film = nullptr;       // [B][F]
  float* time_buf = nullptr;   // [B] direct time values
  int* step_ctr = nullptr;
  DevBuf table;                // float [kUpdateCols][table_cap]: the step table of the loop in flight (UpdateArgs::tab)
  int table_cap = 0;
  unsigned* handoff_timeouts = nullptr;        // device counter: bounded FULL / FREE spins of k_conv_ws that gave up (0 in a correct run)
  unsigned long long* loop_params = nullptr;   // device {seed, noise address}: per-call values the captured step reads
  DevBuf sample_ids;                           // device uint64 [B], allocated by the first loop with per-sample noise streams and
                                               // kept: a captured step holds its address, every call writes its ids there
  // few-step solvers (dsx_solver_loop): allocated by the first such call, outside the workspace, and kept like sample_ids
  DevBuf solver_hist;                          // the previous step's predicted x0, NHWC fp32 [B][H][W][x_c]
  // per-call host data (step table, seed, noise address) is staged in pinned memory, one slot per call in flight: a
  // slot is reused only after the event recorded behind its copies has completed, so a second dsx_sample_loop on the
  // same executor never overwrites bytes an earlier call's asynchronous copy has yet to read
  struct Staging { PinnedBuf host; size_t floats = 0; Event ev; bool busy = false; };
  Staging staging[4];
  int staging_next = 0;
  hipStream_t last_stream = nullptr;           // stream of the most recent graph launches
  // graph
  Graph graph;
  std::vector<float> graph_sig;
  // time predictor head
  DevBuf tp_w;                 // float: weights [49][in], then the bias and the mask (tp_b, tp_mask point into it)
  float* tp_b = nullptr; float* tp_mask = nullptr;
  int launches = 0;
  std::vector<dsx_layer_info> layers;   // layer table (dsx_exec_layer_info): recorded by the planning pass only
};

// ------------------------------------------------------------------ functions called across files
namespace dsx {
// dsx_model.cpp
void conv_geometry(int cout, int cin, int ks, int dtype, int& kchunks, int& nblocks);
// dsx_plan.cpp
PlanKnobs read_plan_knobs();
int run_planner(dsx_exec* ex, char* fake_base, size_t* sizing_bytes);
hipError_t launch_op(const PlanOp& o, hipStream_t st);
// dsx_exec.cpp
std::unique_ptr<dsx_exec> new_exec(dsx_model* m, int B, int H, int W, int cond_channels);
// dsx_eval.cpp
int norm4_ok(const double norm[4]);
}  // namespace dsx
