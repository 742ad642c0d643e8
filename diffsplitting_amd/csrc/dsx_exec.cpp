// dsx_exec.cpp — the executor: life cycle and introspection, the profiling entry points, the UNet forward, the
// graph-captured sampling loop, single steps and the time-predictor head.  C ABI in include/dsx.h.
#include "dsx_rt.h"

// ------------------------------------------------------------------ executor
// An executor of `m` for (B, H, W) that has yet to be planned: knobs read, conv_naive taken from the model.
std::unique_ptr<dsx_exec> dsx::new_exec(dsx_model* m, int B, int H, int W, int cond_channels) {
  auto ex = std::make_unique<dsx_exec>();
  ex->m = m; ex->B = B; ex->H = H; ex->W = W;
  ex->knobs = read_plan_knobs();
  ex->knobs.conv_naive = m->want_naive;   // the model's device image decides (naive weights exist only then)
  ex->cond_c = cond_channels; ex->x_c = m->cfg.in_channel - cond_channels;
  return ex;
}

extern "C" int dsx_exec_create(dsx_model* m, int B, int H, int W, int cond_channels, dsx_exec** out) {
  if (!m || !out || B < 1 || H < 1 || W < 1) return fail(DSX_ERR_INVALID, "bad argument");
  if (!m->finalized) return fail(DSX_ERR_STATE, "dsx_model_finalize must precede dsx_exec_create");
  if (cond_channels < 0 || cond_channels >= m->cfg.in_channel) return fail(DSX_ERR_INVALID, "bad cond_channels");
  HIP_TRY(conv_init());
  HIP_TRY(ops_init());
  auto ex = new_exec(m, B, H, W, cond_channels);
  const int rc = run_planner(ex.get(), nullptr, nullptr);
  if (rc) return rc;
  if (hipMemset(ex->step_ctr, 0, 256) != hipSuccess) return fail(DSX_ERR_HIP, "hipMemset failed");
  *out = ex.release();
  return DSX_OK;
}

// Drops the captured graph.  An executable graph may still have launches queued: wait for them before destroying it.
static int drop_graph(dsx_exec* ex) {
  if (ex->graph.exec && ex->last_stream) HIP_TRY(hipStreamSynchronize(ex->last_stream));
  ex->graph.reset();
  return DSX_OK;
}

extern "C" void dsx_exec_destroy(dsx_exec* ex) {
  if (!ex) return;
  for (auto& sl : ex->staging)   // a pinned slot an asynchronous copy has yet to read
    if (sl.busy) (void)hipEventSynchronize(sl.ev.e);
  (void)drop_graph(ex);
  delete ex;
}
extern "C" size_t dsx_exec_workspace_bytes(const dsx_exec* ex) { return ex ? ex->ws_bytes : 0; }
// Bounded spins of the conv kernel's loader -> compute hand-off (three-image tiles) that gave up since the executor was
// created: 0 in every correct run; anything else means wrong pixels were produced.  Synchronises the device.
extern "C" int dsx_exec_handoff_timeouts(dsx_exec* ex, unsigned* count) {
  if (!ex || !count) return fail(DSX_ERR_INVALID, "null argument");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(count, ex->handoff_timeouts, sizeof(unsigned), hipMemcpyDeviceToHost));
  return DSX_OK;
}
extern "C" int dsx_exec_num_launches(const dsx_exec* ex) { return ex ? ex->launches : 0; }

extern "C" int dsx_exec_num_ops(const dsx_exec* ex) { return ex ? (int)ex->ops.size() : 0; }
extern "C" int dsx_exec_num_layers(const dsx_exec* ex) { return ex ? (int)ex->layers.size() : 0; }
extern "C" int dsx_exec_layer_info(const dsx_exec* ex, int i, dsx_layer_info* info) {
  if (!ex || !info || i < 0 || i >= (int)ex->layers.size()) return fail(DSX_ERR_INVALID, "bad layer index");
  *info = ex->layers[i];
  return DSX_OK;
}
extern "C" int dsx_exec_copy_workspace(const dsx_exec* ex, uint64_t src, size_t bytes, void* dst, void* stream) {
  if (!ex || !dst) return fail(DSX_ERR_INVALID, "null argument");
  const uint64_t lo = (uint64_t)(uintptr_t)ex->ws, hi = lo + ex->ws_bytes;
  if (!ex->ws || src < lo || src > hi || bytes > hi - src) return fail(DSX_ERR_INVALID, "range is not inside the workspace");
  HIP_TRY(hipMemcpyAsync(dst, (const void*)(uintptr_t)src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_exec_op_info(const dsx_exec* ex, int i, char* desc, int cap, int* kind, double* flops,
                                double* bytes) {
  if (!ex || i < 0 || i >= (int)ex->ops.size()) return fail(DSX_ERR_INVALID, "bad op index");
  const PlanOp& o = ex->ops[i];
  if (desc && cap > 0) snprintf(desc, cap, "%s", o.desc.c_str());
  if (kind) *kind = o.kind;
  if (flops) *flops = o.flops;
  if (bytes) *bytes = o.bytes;
  return DSX_OK;
}
// diagnostics: the launches of one kind (DSX_OP_*) captured into a graph of their own and replayed `iters` times;
// *ms_per_replay = mean time of a replay, *launches = how many launches it holds
extern "C" int dsx_exec_time_kind(dsx_exec* ex, int kind, int iters, float* ms_per_replay, int* launches,
                                  void* stream) {
  if (!ex || !ms_per_replay || iters < 1) return fail(DSX_ERR_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (!st) return fail(DSX_ERR_INVALID, "dsx_exec_time_kind needs a non-default stream (stream capture)");
  // kind >= 0: the launches of that kind; -1: every launch of the forward; <= -2: every launch except kind (-kind - 2)
  auto selected = [&](int k) { return kind >= 0 ? k == kind : (kind == -1 ? true : k != -kind - 2); };
  int n = 0;
  for (auto& op : ex->ops) n += selected(op.kind) ? 1 : 0;
  if (launches) *launches = n;
  if (n == 0) { *ms_per_replay = 0.f; return DSX_OK; }
  Graph g;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  hipError_t err = hipSuccess;
  for (size_t i = 0; i < ex->ops.size() && err == hipSuccess; ++i)
    if (selected(ex->ops[i].kind)) err = launch_op(ex->ops[i], st);
  hipError_t e2 = hipStreamEndCapture(st, &g.graph);
  if (err != hipSuccess || e2 != hipSuccess || !g.graph)
    return fail(DSX_ERR_HIP, "capture of the kernel family failed: %s", hipGetErrorString(err != hipSuccess ? err : e2));
  HIP_TRY(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
  Event e0, e1;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  HIP_TRY(hipGraphLaunch(g.exec, st));   // warm-up replay
  HIP_TRY(hipEventRecord(e0.e, st));
  for (int it = 0; it < iters; ++it) HIP_TRY(hipGraphLaunch(g.exec, st));
  HIP_TRY(hipEventRecord(e1.e, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
  *ms_per_replay = ms / iters;
  return DSX_OK;
}

// diagnostics: copy the 128 in-kernel stamps of the launch chosen with DSX_STAMP_OP (zeros if none)
extern "C" int dsx_exec_read_stamps(dsx_exec* ex, unsigned long long* out128) {
  if (!ex || !out128) return fail(DSX_ERR_INVALID, "null argument");
  memset(out128, 0, 128 * 8);
  if (!ex->stamp_buf) return DSX_OK;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out128, ex->stamp_buf, 128 * 8, hipMemcpyDeviceToHost));
  return DSX_OK;
}

// Eager, event-timed replay of the UNet plan on `stream` (inputs: whatever the
// buffers hold).  ms_per_op[i] = mean over `iters` of the hipEvent time around launch i.
extern "C" int dsx_exec_profile(dsx_exec* ex, int iters, float* ms_per_op, void* stream) {
  if (!ex || !ms_per_op || iters < 1) return fail(DSX_ERR_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t n = ex->ops.size();
  std::vector<Event> ev(2 * n);
  for (auto& e : ev) HIP_TRY(e.create());
  std::vector<double> acc(n, 0.0);
  for (int it = 0; it < iters; ++it) {
    static const bool trace = getenv("DSX_TRACE") != nullptr;   // debugging: name each launch, sync after it
    for (size_t i = 0; i < n; ++i) {
      if (trace) { fprintf(stderr, "[dsx] op %zu: %s\n", i, ex->ops[i].desc.c_str()); fflush(stderr); }
      HIP_TRY(hipEventRecord(ev[2 * i].e, st));
      HIP_TRY(launch_op(ex->ops[i], st));
      HIP_TRY(hipEventRecord(ev[2 * i + 1].e, st));
      if (trace) HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; ++i) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ev[2 * i].e, ev[2 * i + 1].e));
      acc[i] += ms;
    }
  }
  for (size_t i = 0; i < n; ++i) ms_per_op[i] = (float)(acc[i] / iters);
  return DSX_OK;
}

// time embedding + UNet body on `st`; inputs already in ex->in_cond / ex->in_x
static int run_unet(dsx_exec* ex, bool from_table, int n_time, hipStream_t st, int per_sample = 0) {
  dsx_model* m = ex->m;
  if (m->cfg.with_time_emb) {
    TembArgs t{};
    t.flavour = m->cfg.flavour; t.B = ex->B; t.n_time = n_time;
    t.time = from_table ? nullptr : ex->time_buf;
    t.table = ex->table.as<float>(); t.step_ctr = ex->step_ctr; t.per_sample = per_sample;
    t.inner = m->cfg.inner_channel; t.freq = m->d_freq;
    t.w1 = m->d_w1; t.b1 = m->d_b1; t.w2 = m->d_w2; t.b2 = m->d_b2;
    t.wf = m->d_wf; t.bf = m->d_bf; t.F = m->F; t.film = ex->film;
    HIP_TRY(launch_temb(t, st));
  }
  for (auto& op : ex->ops) HIP_TRY(launch_op(op, st));
  return DSX_OK;
}

static int load_inputs(dsx_exec* ex, const float* cond_nchw, const float* x_nchw, int x_total_c,
                       int x_c_off, hipStream_t st);

extern "C" int dsx_unet_forward(dsx_exec* ex, const float* x, const float* time, int n_time, float* y,
                                void* stream) {
  if (!ex || !x || !y) return fail(DSX_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  dsx_model* m = ex->m;
  if (m->cfg.with_time_emb) {
    if (!time || !(n_time == 1 || n_time == ex->B)) return fail(DSX_ERR_INVALID, "n_time must be 1 or B");
    HIP_TRY(hipMemcpyAsync(ex->time_buf, time, (size_t)n_time * 4, hipMemcpyDeviceToDevice, st));
  }
  // x is (B, in_channel, H, W): channels [0,cond_c) feed the cond tensor, the rest the state tensor
  int rc = load_inputs(ex, ex->cond_c ? x : nullptr, x, m->cfg.in_channel, ex->cond_c, st);
  if (rc) return rc;
  if ((rc = run_unet(ex, false, n_time, st))) return rc;
  HIP_TRY(launch_nhwc_to_nchw((const float*)ex->out.p, y, ex->B, ex->out.C, ex->H, ex->W, st));
  return DSX_OK;
}

static int load_inputs(dsx_exec* ex, const float* cond_nchw, const float* x_nchw, int x_total_c,
                       int x_c_off, hipStream_t st) {
  const int HW = ex->H * ex->W;
  if (ex->cond_c) {
    if (!cond_nchw) return fail(DSX_ERR_INVALID, "this executor was created with cond_channels > 0");
    const int ctot = (cond_nchw == x_nchw) ? x_total_c : ex->cond_c;
    HIP_TRY(dsx::launch_nchw_slice_to_nhwc(cond_nchw, ex->in_cond.p, ex->in_cond.st, ex->B, ex->cond_c, ctot,
                                           0, HW, st));
  }
  HIP_TRY(dsx::launch_nchw_slice_to_nhwc(x_nchw, ex->in_x.p, ex->in_x.st, ex->B, ex->x_c, x_total_c, x_c_off,
                                         HW, st));
  if (ex->in_x.st)   // the sampler state itself stays fp32
    HIP_TRY(dsx::launch_nchw_slice_to_nhwc(x_nchw, ex->x_state, 0, ex->B, ex->x_c, x_total_c, x_c_off, HW, st));
  return DSX_OK;
}

// ------------------------------------------------------------------ sampler
// the device table [kUpdateCols][cap] holds T values per column
static int ensure_table(dsx_exec* ex, int T) {
  if (T > ex->table_cap) {
    // the table's column stride (= capacity) is baked into captured graphs: drop them
    const int rc = drop_graph(ex);
    if (rc) return rc;
    const int cap = std::max(T, 2048);
    HIP_TRY(ex->table.alloc((size_t)kUpdateCols * cap * sizeof(float)));
    ex->table_cap = cap;
  }
  return DSX_OK;
}

// a pinned staging slot holding this call's table [kUpdateCols][cap] (T values per column; a null column stays zero)
// followed by {seed, noise address} and, with per-sample noise streams, the B sample ids; *out = its host pointer
static int stage_call(dsx_exec* ex, const float* const* cols, int T, uint64_t seed, const float* noise,
                      const uint64_t* ids, dsx_exec::Staging** out) {
  const int ncols = kUpdateCols, cap = ex->table_cap;
  const size_t need = (size_t)ncols * cap + 4 + (ids ? (size_t)2 * ex->B : 0);   // + 16 bytes of loop parameters (+ ids)
  dsx_exec::Staging& sl = ex->staging[ex->staging_next];
  ex->staging_next = (ex->staging_next + 1) % 4;
  if (sl.busy) { HIP_TRY(hipEventSynchronize(sl.ev.e)); sl.busy = false; }
  if (sl.floats < need) {
    sl.floats = 0;
    HIP_TRY(sl.host.alloc(need * sizeof(float)));
    sl.floats = need;
  }
  if (!sl.ev.e) HIP_TRY(sl.ev.create(hipEventDisableTiming));
  float* host = sl.host.as<float>();
  memset(host, 0, (size_t)ncols * cap * sizeof(float));
  for (int k = 0; k < ncols; ++k)
    if (cols[k]) memcpy(host + (size_t)k * cap, cols[k], (size_t)T * 4);
  unsigned long long lp[2] = {seed, (unsigned long long)(uintptr_t)noise};
  memcpy(host + (size_t)ncols * cap, lp, 16);
  if (ids) memcpy(host + (size_t)ncols * cap + 4, ids, (size_t)ex->B * 8);
  *out = &sl;
  return DSX_OK;
}
// the staged call -> device memory on `st`: the table, the loop parameters, the ids, the step counter
static int upload_call(dsx_exec* ex, dsx_exec::Staging* sl, bool ids, hipStream_t st) {
  const int ncols = kUpdateCols, cap = ex->table_cap;
  const float* host = sl->host.as<float>();
  HIP_TRY(hipMemcpyAsync(ex->table.p, host, (size_t)ncols * cap * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ex->loop_params, host + (size_t)ncols * cap, 16, hipMemcpyHostToDevice, st));
  if (ids)
    HIP_TRY(hipMemcpyAsync(ex->sample_ids.p, host + (size_t)ncols * cap + 4, (size_t)ex->B * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(sl->ev.e, st));
  sl->busy = true;
  HIP_TRY(hipMemsetAsync(ex->step_ctr, 0, 4, st));
  return DSX_OK;
}

// what a captured step bakes in (not the step count, the seed, the noise address or the sample ids): also the graph's
// signature, so a DDIM table through dsx_sample_loop and through dsx_solver_loop capture separate graphs
struct LoopMode {
  int predict_eps, clip, per_sample;
  int history;        // the few-step solvers' x0 history (ex->solver_hist) is read and written
  int use_noise, streams;
  std::vector<float> sig() const {
    return {(float)predict_eps, (float)clip, (float)use_noise, (float)per_sample, (float)streams, (float)history};
  }
};
static int enqueue_step(dsx_exec* ex, const LoopMode& m, hipStream_t st) {
  int rc = run_unet(ex, true, m.per_sample ? ex->B : 1, st, m.per_sample);
  if (rc) return rc;
  UpdateArgs u{};
  u.x = ex->x_state; u.x_act = ex->in_x.st ? ex->in_x.p : nullptr; u.x_act_kind = ex->in_x.st;
  u.net = (const float*)ex->out.p; u.x0_hist = m.history ? ex->solver_hist.as<float>() : nullptr;
  u.use_noise = m.use_noise; u.loop_params = ex->loop_params;
  u.tab = ex->table.as<float>(); u.n_steps = ex->table_cap; u.step_ctr = ex->step_ctr;
  u.predict_eps = m.predict_eps; u.clip = m.clip; u.per_sample = m.per_sample;
  u.B = ex->B; u.C = ex->x_c; u.H = ex->H; u.W = ex->W;
  u.sample_ids = m.streams ? ex->sample_ids.as<unsigned long long>() : nullptr;   // the executor's buffer, not the ids
  HIP_TRY(launch_update(u, st));
  HIP_TRY(launch_advance(ex->step_ctr, st));
  return DSX_OK;
}

// T steps on `st` from the loaded inputs, snapshots after the named ones, the final state to `x`.  use_graph: `step` is
// captured once into ex->graph and replayed; a kept graph is replayed only when its signature equals `sig`, so loops
// whose steps differ (other mode flags, another kernel) recapture instead of replaying each other's step.
template <class Step>
static int replay_steps(dsx_exec* ex, const std::vector<float>& sig, Step&& step, int T, const int32_t* snap_steps, int n_snap,
                        float* snaps, float* x, int use_graph, hipStream_t st) {
  int rc = DSX_OK;
  const size_t snap_elems = (size_t)ex->B * ex->x_c * ex->H * ex->W;
  bool graph_ok = false;
  if (use_graph) {
    if (!ex->graph.exec || sig != ex->graph_sig) {
      if ((rc = drop_graph(ex))) return rc;
      Stream cs;
      HIP_TRY(cs.create(hipStreamNonBlocking));
      hipError_t e = hipStreamBeginCapture(cs.s, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        rc = step(cs.s);
        hipError_t e2 = hipStreamEndCapture(cs.s, &ex->graph.graph);
        if (rc == DSX_OK && e2 == hipSuccess) e2 = hipGraphInstantiate(&ex->graph.exec, ex->graph.graph, nullptr, nullptr, 0);
        if (rc != DSX_OK || e2 != hipSuccess) {
          (void)hipGetLastError();
          ex->graph.reset();
        }
      } else {
        (void)hipGetLastError();
      }
      if (ex->graph.exec) ex->graph_sig = sig;
      else if (rc != DSX_OK) return rc;
    }
    graph_ok = ex->graph.exec != nullptr;
    if (!graph_ok) return fail(DSX_ERR_HIP, "hipGraph capture of the sampling step failed");
    ex->last_stream = st;
  }
  int snap_i = 0;
  for (int s = 0; s < T; ++s) {
    if (graph_ok) HIP_TRY(hipGraphLaunch(ex->graph.exec, st));
    else if ((rc = step(st))) return rc;
    while (snap_i < n_snap && snap_steps[snap_i] == s) {
      HIP_TRY(launch_nhwc_to_nchw(ex->x_state, snaps + (size_t)snap_i * snap_elems, ex->B, ex->x_c, ex->H,
                                  ex->W, st));
      ++snap_i;
    }
  }
  HIP_TRY(launch_nhwc_to_nchw(ex->x_state, x, ex->B, ex->x_c, ex->H, ex->W, st));
  return DSX_OK;
}

// The loop behind dsx_sample_loop, dsx_sample_loop_streams and dsx_solver_loop, which check their own arguments.
// cols: the kUpdateCols host columns in the table's order, `rows` values each (a null column counts as zeros); T steps.
// ids == nullptr: the default noise (one stream per step at the flat batch index); else B sample ids.
static int run_loop(dsx_exec* ex, const float* const* cols, int T, int rows, LoopMode m, const float* cond, float* x,
                    const float* noise, uint64_t seed, const uint64_t* ids, const int32_t* snap_steps, int n_snap,
                    float* snaps, int use_graph, hipStream_t st) {
  if (m.history && m.per_sample) return fail(DSX_ERR_INVALID, "x0 history with a per_sample table");
  m.use_noise = noise ? 1 : 0; m.streams = ids ? 1 : 0;
  int rc = ensure_table(ex, rows);
  if (rc) return rc;
  // once each, outside the workspace: captured steps keep the addresses
  if (m.history && !ex->solver_hist.p) HIP_TRY(ex->solver_hist.alloc((size_t)ex->B * ex->x_c * ex->H * ex->W * sizeof(float)));
  if (ids && !ex->sample_ids.p) HIP_TRY(ex->sample_ids.alloc((size_t)ex->B * 8));
  // per-call values (step table; seed, noise address: the captured step does not bake them in) go to device memory
  // from a pinned staging slot of this call's own
  dsx_exec::Staging* sl = nullptr;
  if ((rc = stage_call(ex, cols, rows, seed, noise, ids, &sl))) return rc;
  if ((rc = upload_call(ex, sl, ids != nullptr, st))) return rc;
  if ((rc = load_inputs(ex, cond, x, ex->x_c, 0, st))) return rc;
  return replay_steps(ex, m.sig(), [&](hipStream_t s) { return enqueue_step(ex, m, s); }, T, snap_steps, n_snap, snaps, x,
                      use_graph, st);
}

static int sample_loop(dsx_exec* ex, const dsx_step_table* tab, const float* cond, float* x, const float* noise,
                       uint64_t seed, const int32_t* snap_steps, int n_snap, float* snaps, int use_graph, void* stream,
                       const uint64_t* ids) {
  if (!ex || !tab || !x || tab->n_steps < 1) return fail(DSX_ERR_INVALID, "bad argument");
  if (!tab->tcond || !tab->c1 || !tab->c2 || !tab->sigma || (tab->predict_eps && (!tab->a || !tab->b)))
    return fail(DSX_ERR_INVALID, "step table columns missing");
  if (ex->out.C != ex->x_c)
    return fail(DSX_ERR_INVALID, "UNet out_channel (%d) must equal the state channels (%d)", ex->out.C, ex->x_c);
  if (n_snap > 0 && (!snap_steps || !snaps)) return fail(DSX_ERR_INVALID, "snapshot arrays missing");
  if (tab->per_sample != 0 && tab->per_sample != ex->B)
    return fail(DSX_ERR_INVALID, "per_sample step table for %d samples, executor batch %d", tab->per_sample, ex->B);
  const float* cols[kUpdateCols] = {tab->tcond, tab->a, tab->b, tab->c1, tab->c2, nullptr, tab->sigma};   // cp: zeros
  const int per = tab->per_sample > 0 ? tab->per_sample : 1;
  const LoopMode m{tab->predict_eps, tab->clip, tab->per_sample > 0 ? 1 : 0, 0, 0, 0};
  return run_loop(ex, cols, tab->n_steps, tab->n_steps * per, m, cond, x, noise, seed, ids, snap_steps, n_snap, snaps,
                  use_graph, (hipStream_t)stream);
}

extern "C" int dsx_sample_loop(dsx_exec* ex, const dsx_step_table* tab, const float* cond, float* x,
                               const float* noise, uint64_t seed, const int32_t* snap_steps, int n_snap,
                               float* snaps, int use_graph, void* stream) {
  return sample_loop(ex, tab, cond, x, noise, seed, snap_steps, n_snap, snaps, use_graph, stream, nullptr);
}

// ---- per-sample noise streams (include/dsx.h): the sample stream (seed, id, draw) is the stream (seed, id << 24 | draw)
static int stream_ids_ok(const char* what, const uint64_t* ids, int n_ids, int B, uint64_t draw_last) {
  if (!ids) return fail(DSX_ERR_INVALID, "%s: sample_ids is null", what);
  if (n_ids != B) return fail(DSX_ERR_INVALID, "%s: %d sample ids for a batch of %d", what, n_ids, B);
  if (draw_last >= DSX_STREAM_DRAW_LIMIT)
    return fail(DSX_ERR_INVALID, "%s: draw ordinal %llu out of range (draw < 2^24)", what, (unsigned long long)draw_last);
  for (int b = 0; b < B; ++b)
    if (ids[b] >= DSX_STREAM_ID_LIMIT)
      return fail(DSX_ERR_INVALID, "%s: sample id %llu (entry %d) out of range (id < 2^40)", what, (unsigned long long)ids[b], b);
  return DSX_OK;
}

extern "C" int dsx_sample_loop_streams(dsx_exec* ex, const dsx_step_table* tab, const float* cond, float* x,
                                       const float* noise, uint64_t seed, const int32_t* snap_steps, int n_snap,
                                       float* snaps, int use_graph, void* stream, const uint64_t* sample_ids,
                                       int n_sample_ids) {
  if (!ex || !tab) return fail(DSX_ERR_INVALID, "sample_loop_streams: null executor or step table");
  if (noise) return fail(DSX_ERR_INVALID, "sample_loop_streams: injected noise together with sample_ids");
  const int rc = stream_ids_ok("sample_loop_streams", sample_ids, n_sample_ids, ex->B, (uint64_t)std::max(tab->n_steps, 0));
  if (rc) return rc;
  return sample_loop(ex, tab, cond, x, nullptr, seed, snap_steps, n_snap, snaps, use_graph, stream, sample_ids);
}

// ---- few-step solvers (include/dsx.h): the same loop with the x0 history; step_update's c1 = c0, c2 = cx
extern "C" int dsx_solver_loop(dsx_exec* ex, const dsx_solver_table* tab, const float* cond, float* x, const float* noise,
                               uint64_t seed, const int32_t* snap_steps, int n_snap, float* snaps, int use_graph,
                               void* stream, const uint64_t* sample_ids, int n_sample_ids) {
  if (!ex) return fail(DSX_ERR_INVALID, "solver_loop: null executor");
  if (!tab) return fail(DSX_ERR_INVALID, "solver_loop: null solver table");
  if (!x || tab->n_steps < 1) return fail(DSX_ERR_INVALID, "solver_loop: null state or empty table");
  if (!tab->tcond || !tab->a || !tab->b || !tab->cx || !tab->c0 || !tab->cp || !tab->sigma)
    return fail(DSX_ERR_INVALID, "solver_loop: solver table columns missing");
  if (tab->cp[0] != 0.f) return fail(DSX_ERR_INVALID, "solver_loop: cp[0] != 0: no previous x0 at the first step");
  if (ex->out.C != ex->x_c)
    return fail(DSX_ERR_INVALID, "solver_loop: UNet out_channel (%d) must equal the state channels (%d)", ex->out.C, ex->x_c);
  if (n_snap > 0 && (!snap_steps || !snaps)) return fail(DSX_ERR_INVALID, "solver_loop: snapshot arrays missing");
  if (sample_ids) {
    if (noise) return fail(DSX_ERR_INVALID, "solver_loop: injected noise together with sample_ids");
    const int rc = stream_ids_ok("solver_loop", sample_ids, n_sample_ids, ex->B, (uint64_t)tab->n_steps);
    if (rc) return rc;
  }
  const float* cols[kUpdateCols] = {tab->tcond, tab->a, tab->b, tab->c0, tab->cx, tab->cp, tab->sigma};
  const LoopMode m{1, tab->clip ? 1 : 0, 0, 1, 0, 0};
  return run_loop(ex, cols, tab->n_steps, tab->n_steps, m, cond, x, noise, seed, sample_ids, snap_steps, n_snap, snaps,
                  use_graph, (hipStream_t)stream);
}

extern "C" int dsx_randn_samples(float* out, int B, int64_t chw, uint64_t seed, const uint64_t* ids, uint32_t draw,
                                 void* stream) {
  if (!out || B < 1 || chw < 1) return fail(DSX_ERR_INVALID, "randn_samples: null output or empty shape (%d, %lld)", B, (long long)chw);
  if ((int64_t)B * chw > ((int64_t)1 << 40)) return fail(DSX_ERR_INVALID, "randn_samples: tensor too large");
  const int rc = stream_ids_ok("randn_samples", ids, B, B, draw);
  if (rc) return rc;
  HIP_TRY(each_stream_chunk(B, ids, draw, [&](int b0, int rows, const StreamIds& s) {   // the ids travel in the kernel arguments
    return launch_randn_samples(out + (size_t)b0 * chw, rows, chw, seed, s, (hipStream_t)stream);
  }));
  return DSX_OK;
}

// ---- single reverse steps: one-row step tables through dsx_sample_loop, no graph (nothing to replay)
extern "C" int dsx_sr3_step(dsx_exec* ex, float noise_level, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1,
                            float coef2, float sigma, int clip_denoised, const float* cond, float* x, const float* noise,
                            uint64_t seed, void* stream) {
  dsx_step_table t{};
  t.n_steps = 1; t.tcond = &noise_level; t.a = &sqrt_recip_ac; t.b = &sqrt_recipm1_ac; t.c1 = &coef1; t.c2 = &coef2;
  t.sigma = &sigma; t.predict_eps = 1; t.clip = clip_denoised ? 1 : 0; t.per_sample = 0;
  return dsx_sample_loop(ex, &t, cond, x, noise, seed, nullptr, 0, nullptr, 0, stream);
}
extern "C" int dsx_indi_step(dsx_exec* ex, float t_cur, float c_x0, float c_xt, float noise_scale, float* x,
                             const float* noise, uint64_t seed, void* stream) {
  dsx_step_table t{};
  t.n_steps = 1; t.tcond = &t_cur; t.c1 = &c_x0; t.c2 = &c_xt; t.sigma = &noise_scale;
  t.predict_eps = 0; t.clip = 0; t.per_sample = 0;
  return dsx_sample_loop(ex, &t, nullptr, x, noise, seed, nullptr, 0, nullptr, 0, stream);
}

extern "C" int dsx_randn(float* out, int64_t n, uint64_t seed, uint64_t subseq, void* stream) {
  if (!out || n < 0) return fail(DSX_ERR_INVALID, "bad argument");
  if (n == 0) return DSX_OK;
  HIP_TRY(launch_randn(out, n, seed, subseq, (hipStream_t)stream));
  return DSX_OK;
}

// ---- the pointwise sampler kernels (dsx_steps.hip) and the loss reduction (dsx_eval.hip)
static int steps_shape(const char* what, int B, int C, int H, int W) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return fail(DSX_ERR_INVALID, "%s: empty shape (%d, %d, %d, %d)", what, B, C, H, W);
  if ((int64_t)H * W > INT32_MAX || (int64_t)B * C * H * W > ((int64_t)1 << 40))
    return fail(DSX_ERR_INVALID, "%s: tensor too large", what);
  return DSX_OK;
}
extern "C" int dsx_q_sample(const float* x0, const float* xe, int B, int C, int Ce, int H, int W, const float* c0,
                            const float* c1, const float* c2, const float* z, uint64_t seed, uint64_t subseq,
                            float* z_out, float* dst, int Cdst, int coff, void* stream) {
  int rc = steps_shape("q_sample", B, C, H, W);
  if (rc) return rc;
  if (xe && (Ce < 1 || C % Ce != 0))
    return fail(DSX_ERR_INVALID, "q_sample: x_end has %d channels, x_start %d: C %% Ce != 0", Ce, C);
  if (coff < 0 || (int64_t)coff + C > Cdst)
    return fail(DSX_ERR_INVALID, "q_sample: channels %d..%d do not fit a destination of %d (coff + C > Cdst)", coff,
                coff + C, Cdst);
  if ((rc = steps_shape("q_sample", B, Cdst, H, W))) return rc;    // the destination may be the wider tensor
  if (!x0 || !c0 || !c2 || !dst || (xe && !c1)) return fail(DSX_ERR_INVALID, "q_sample: null argument");
  QSampleArgs a{x0, xe, c0, c1, c2, z, seed, subseq, z ? nullptr : z_out, dst, B, C, xe ? Ce : 1, H * W, Cdst, coff};
  HIP_TRY(launch_q_sample(a, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_loss_blocks(int C, int H, int W) {
  if (C < 1 || H < 1 || W < 1 || (int64_t)C * H * W > INT32_MAX)
    return fail(DSX_ERR_INVALID, "loss: bad sample shape (%d, %d, %d)", C, H, W);
  return loss_blocks((int64_t)C * H * W);
}
extern "C" int dsx_loss(const float* a, const float* b, int B, int C, int H, int W, int squared, double* partial_dev,
                        double* per_sample_dev, void* stream) {
  const int blocks = dsx_loss_blocks(C, H, W);
  if (blocks < 0) return blocks;
  if (B < 1 || B > 65535) return fail(DSX_ERR_INVALID, "loss: B = %d, must be in 1..65535", B);
  if (!a || !b || !partial_dev || !per_sample_dev) return fail(DSX_ERR_INVALID, "loss: null argument");
  HIP_TRY(launch_loss(a, b, B, (int64_t)C * H * W, squared ? 1 : 0, partial_dev, per_sample_dev, (hipStream_t)stream));
  return DSX_OK;
}

// ---- the fused attention kernel (dsx_attn.hip) on caller tensors: the planner's launch with the layout spelled out
extern "C" int dsx_attention(const void* qkv, int ld, int q_col, int k_col, int v_col, void* out, int ldo, int storage,
                             int B, int L, int C, int col_split, void* stream) {
  if (!qkv || !out) return fail(DSX_ERR_INVALID, "attention: null argument");
  if (storage < 0 || storage > 2) return fail(DSX_ERR_INVALID, "attention: storage kind %d (0 fp32, 1 bf16, 2 fp16)", storage);
  if (!attn_supported(C, L))
    return fail(DSX_ERR_INVALID, "attention: head dimension %d (8..1024, multiple of 8) with %d tokens is not supported", C, L);
  if (B < 1) return fail(DSX_ERR_INVALID, "attention: B = %d", B);
  const int es = storage == 0 ? 4 : 2, epu = 16 / es;          // element size, elements per 16-byte unit
  if (q_col < 0 || k_col < 0 || v_col < 0 || q_col % epu || k_col % epu || v_col % epu)
    return fail(DSX_ERR_INVALID, "attention: column offsets (%d, %d, %d) must be non-negative multiples of %d", q_col,
                k_col, v_col, epu);
  if (ld < 1 || ld % epu) return fail(DSX_ERR_INVALID, "attention: ld = %d is not a multiple of %d", ld, epu);
  if ((int64_t)q_col + C > ld || (int64_t)k_col + C > ld || (int64_t)v_col + C > ld)
    return fail(DSX_ERR_INVALID, "attention: columns (%d, %d, %d) + C = %d do not fit a row of ld = %d", q_col, k_col,
                v_col, C, ld);
  if (k_col < q_col || v_col < q_col)
    return fail(DSX_ERR_INVALID, "attention: k and v must not start before q (offsets are taken relative to q)");
  if (ldo % 4) return fail(DSX_ERR_INVALID, "attention: ldo = %d is not a multiple of 4", ldo);
  if (ldo < C) return fail(DSX_ERR_INVALID, "attention: ldo = %d < C = %d", ldo, C);
  if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 15))
    return fail(DSX_ERR_INVALID, "attention: qkv and out must be 16-byte aligned");
  if ((int64_t)L * ld * es >= ((int64_t)1 << 31))
    return fail(DSX_ERR_INVALID, "attention: one image of %d rows of %d elements does not fit a 2 GiB buffer descriptor", L,
                ld);
  if ((int64_t)B * ((L + 31) / 32) * 2 > INT32_MAX) return fail(DSX_ERR_INVALID, "attention: too many query tiles");
  AttnArgs a{};
  const char* base = (const char*)qkv;
  a.q = base + (size_t)q_col * es; a.k = base + (size_t)k_col * es; a.v = base + (size_t)v_col * es; a.ld = ld;
  a.out = out; a.ldo = ldo; a.storage = storage;
  a.B = B; a.L = L; a.C = C; a.div = sqrtf((float)C); a.inv_div = 1.0f / a.div;
  HIP_TRY(launch_attn(a, col_split != 0, (hipStream_t)stream));
  return DSX_OK;
}

// ---- caller-driven reverse sampling: one update with its intermediates, the start of interpolate
extern "C" int dsx_posterior_step(const float* x, const float* net, int B, int C, int H, int W, const float* a,
                                  const float* b, const float* c1, const float* c2, const float* sigma,
                                  int predict_eps, int clip, const float* z, uint64_t seed, uint64_t subseq,
                                  int repeat_noise, float* x_recon_out, float* mean_out, float* x_out, void* stream) {
  int rc = steps_shape("posterior_step", B, C, H, W);
  if (rc) return rc;
  if (!x || !net || !c1 || !c2 || !sigma) return fail(DSX_ERR_INVALID, "posterior_step: null argument");
  if (predict_eps && (!a || !b)) return fail(DSX_ERR_INVALID, "posterior_step: predict_eps needs the columns a and b");
  if (!x_recon_out && !mean_out && !x_out) return fail(DSX_ERR_INVALID, "posterior_step: every output is null");
  const StepArgs p{x, net, nullptr, a, b, c1, c2, nullptr, sigma, x_out ? z : nullptr, seed, subseq, x_recon_out, mean_out, x_out,
                   B, predict_eps ? 1 : 0, clip ? 1 : 0, repeat_noise ? 1 : 0, (int64_t)C * H * W};
  HIP_TRY(launch_step(p, (int64_t)H * W, nullptr, 0, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_posterior_step_streams(const float* x, const float* net, int B, int C, int H, int W, const float* a,
                                          const float* b, const float* c1, const float* c2, const float* sigma,
                                          int predict_eps, int clip, const float* z, uint64_t seed, uint64_t draw,
                                          int repeat_noise, float* x_recon_out, float* mean_out, float* x_out,
                                          void* stream, const uint64_t* sample_ids, int n_sample_ids) {
  int rc = steps_shape("posterior_step_streams", B, C, H, W);
  if (rc) return rc;
  if (z) return fail(DSX_ERR_INVALID, "posterior_step_streams: injected noise together with sample_ids");
  if (repeat_noise) return fail(DSX_ERR_INVALID, "posterior_step_streams: repeat_noise together with sample_ids");
  if ((rc = stream_ids_ok("posterior_step_streams", sample_ids, n_sample_ids, B, draw))) return rc;
  if (!x || !net || !c1 || !c2 || !sigma) return fail(DSX_ERR_INVALID, "posterior_step_streams: null argument");
  if (predict_eps && (!a || !b)) return fail(DSX_ERR_INVALID, "posterior_step_streams: predict_eps needs the columns a and b");
  if (!x_recon_out && !mean_out && !x_out) return fail(DSX_ERR_INVALID, "posterior_step_streams: every output is null");
  const StepArgs p{x, net, nullptr, a, b, c1, c2, nullptr, sigma, nullptr, seed, 0, x_recon_out, mean_out, x_out,
                   B, predict_eps ? 1 : 0, clip ? 1 : 0, 0, (int64_t)C * H * W};
  HIP_TRY(launch_step(p, (int64_t)H * W, sample_ids, draw, (hipStream_t)stream));
  return DSX_OK;
}
// one solver update: step_update's c1 = c0, c2 = cx.  sample_ids == nullptr -> z_dev or the stream (seed, subsequence);
// else the sample streams (seed, sample_ids[b], draw)
extern "C" int dsx_solver_step(const float* x, const float* net, const float* x0_prev, int B, int C, int H, int W,
                               const float* a, const float* b, const float* cx, const float* c0, const float* cp,
                               const float* sigma, int clip, const float* z, uint64_t seed, uint64_t subsequence,
                               float* x_recon_out, float* x_out, void* stream, const uint64_t* sample_ids,
                               int n_sample_ids, uint32_t draw) {
  int rc = steps_shape("solver_step", B, C, H, W);
  if (rc) return rc;
  if (sample_ids) {
    if (z) return fail(DSX_ERR_INVALID, "solver_step: injected noise together with sample_ids");
    if ((rc = stream_ids_ok("solver_step", sample_ids, n_sample_ids, B, draw))) return rc;
  }
  if (!x || !net || !a || !b || !cx || !c0 || !sigma) return fail(DSX_ERR_INVALID, "solver_step: null argument");
  if (x0_prev && !cp) return fail(DSX_ERR_INVALID, "solver_step: x0_prev without the column cp");
  if (!x_recon_out || !x_out) return fail(DSX_ERR_INVALID, "solver_step: null output");
  const StepArgs p{x, net, x0_prev, a, b, c0, cx, cp, sigma, z, seed, subsequence, x_recon_out, nullptr, x_out,
                   B, 1, clip ? 1 : 0, 0, (int64_t)C * H * W};
  HIP_TRY(launch_step(p, (int64_t)H * W, sample_ids, draw, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_interp_start(const float* x1, const float* x2, int B, int C, int H, int W, const float* a0,
                                const float* s0, float c, float d, const float* z1, const float* z2, uint64_t seed,
                                uint64_t subseq, float* out, void* stream) {
  int rc = steps_shape("interp_start", B, C, H, W);
  if (rc) return rc;
  if (!x1 || !x2 || !a0 || !s0 || !out) return fail(DSX_ERR_INVALID, "interp_start: null argument");
  if ((z1 == nullptr) != (z2 == nullptr))
    return fail(DSX_ERR_INVALID, "interp_start: both draws are injected, or neither");
  InterpStartArgs p{x1, x2, a0, s0, z1, z2, seed, subseq, c, d, out, B, (int64_t)C * H * W};
  HIP_TRY(launch_interp_start(p, (int64_t)H * W, (hipStream_t)stream));
  return DSX_OK;
}

// ------------------------------------------------------------------ time predictor head
extern "C" int dsx_time_predictor_set_mask(dsx_exec* ex, const float* w, const float* b) {
  if (!ex || !w || !b) return fail(DSX_ERR_INVALID, "null argument");
  const int cin = ex->m->cfg.in_channel;
  if (ex->out.C != 1) return fail(DSX_ERR_INVALID, "TimePredictor head expects out_channel == 1");
  const size_t nw = (size_t)49 * cin;
  std::vector<float> hw(nw);
  for (int ci = 0; ci < cin; ++ci)
    for (int t = 0; t < 49; ++t) hw[(size_t)t * cin + ci] = w[(size_t)ci * 49 + t];  // (1,in,7,7) -> [49][in]
  if (!ex->tp_w.p) HIP_TRY(ex->tp_w.alloc((nw + 64) * 4 + (size_t)ex->B * ex->H * ex->W * 4));
  ex->tp_b = ex->tp_w.as<float>() + nw;
  ex->tp_mask = ex->tp_w.as<float>() + nw + 64;
  HIP_TRY(hipMemcpy(ex->tp_w.p, hw.data(), nw * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ex->tp_b, b, 4, hipMemcpyHostToDevice));
  return DSX_OK;
}

extern "C" int dsx_time_predictor_forward(dsx_exec* ex, const float* x, float* t_out, void* stream) {
  if (!ex || !x || !t_out) return fail(DSX_ERR_INVALID, "null argument");
  if (!ex->tp_w.p) return fail(DSX_ERR_STATE, "dsx_time_predictor_set_mask first");
  hipStream_t st = (hipStream_t)stream;
  int rc = load_inputs(ex, nullptr, x, ex->m->cfg.in_channel, 0, st);
  if (rc) return rc;
  if ((rc = run_unet(ex, false, 1, st))) return rc;
  NaiveConvArgs na{};
  na.c.src0 = ex->in_x.p; na.c.C0 = ex->x_c; na.c.C1 = 0;
  na.c.act_bf16 = ex->in_x.st; na.c.out_bf16 = 0;
  na.c.B = ex->B; na.c.Hs = ex->H; na.c.Ws = ex->W; na.c.Ho = ex->H; na.c.Wo = ex->W;
  na.c.bias = ex->tp_b; na.c.out = ex->tp_mask; na.c.out_ld = 1; na.c.Cout = 1;
  na.w = ex->tp_w.as<float>(); na.ks = 7; na.stride = 1; na.sigmoid_out = 1;
  HIP_TRY(launch_conv_naive(na, st));
  HIP_TRY(launch_masked_mean((const float*)ex->out.p, ex->tp_mask, ex->B, (long long)ex->H * ex->W, t_out, st));
  return DSX_OK;
}
