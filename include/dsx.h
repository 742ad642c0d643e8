/*
 * dsx.h — C ABI of libdsx.so, the MI355X (gfx950) sampling engine that sits
 * underneath the DiffSplitting Python entry points.
 *
 * The reference (rayanirban/DiffSplitting) has no native/FFI layer: its
 * boundary is the Python API in model/networks.py:91 (define_G),
 * model/model.py:63 (DDPM.test) and the sampler classes.  The entry points
 * below are what a native replacement for that hot path binds; each one cites
 * the reference interface it replaces.  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions: every function returns 0 on success and a negative dsx_status
 * on failure; dsx_last_error() returns a thread-local message.  Nothing throws
 * across the ABI.  "dev" pointers are device (HBM) pointers borrowed from the
 * caller (e.g. torch.Tensor.data_ptr()); "host" pointers are plain host
 * memory.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Calls on one handle are not concurrent; distinct handles may run on distinct
 * streams concurrently.  One process drives one GPU.
 */
#ifndef DSX_H
#define DSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSX_ABI_VERSION 2

typedef enum dsx_status {
  DSX_OK = 0,
  DSX_ERR_INVALID = -1,   /* bad argument / shape the kernels do not support */
  DSX_ERR_HIP = -2,       /* a HIP runtime call failed (no device, OOM, ...) */
  DSX_ERR_STATE = -3,     /* call order violated (e.g. forward before finalize) */
  DSX_ERR_MISSING = -4    /* a parameter was never set */
} dsx_status;

const char* dsx_last_error(void);
int dsx_abi_version(void);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int dsx_device_count(void);

/* ------------------------------------------------------------------ UNet */

enum { DSX_FLAVOUR_SR3 = 0, DSX_FLAVOUR_DDPM = 1 };
/* MFMA operand type = activation storage type in HBM; accumulation, GroupNorm statistics and the sampler state are
 * always f32.  F16 is what config/splitting_hagen_indi_joint.json is quoted on (BASELINE "fp16"). */
enum { DSX_DTYPE_F32 = 0, DSX_DTYPE_BF16 = 1, DSX_DTYPE_F16 = 2 };

/* Mirrors the keyword arguments of UNet.__init__
 * (model/sr3_modules/unet.py:161-174, model/ddpm_modules/unet.py:150-162). */
typedef struct dsx_unet_cfg {
  int32_t flavour;          /* DSX_FLAVOUR_* : gamma (sr3) or t (ddpm) conditioning */
  int32_t in_channel;
  int32_t out_channel;
  int32_t inner_channel;
  int32_t norm_groups;
  int32_t n_mults;
  int32_t channel_mults[8];
  int32_t n_attn_res;
  int32_t attn_res[8];
  int32_t res_blocks;
  int32_t image_size;       /* only used to place attn_res, as in the reference */
  int32_t with_time_emb;    /* 0 for the TimePredictor's UNet (time_predictor.py:24-33) */
} dsx_unet_cfg;

typedef struct dsx_model dsx_model;

/* Host-only: builds the topology and the parameter table.  Works without a GPU. */
int dsx_model_create(const dsx_unet_cfg* cfg, dsx_model** out);
void dsx_model_destroy(dsx_model* m);

/* The parameter table uses the reference's state_dict key names relative to
 * the UNet (e.g. "downs.1.res_block.block1.block.3.weight"), in state_dict
 * order, so a *_gen.pth (model/model.py:131-173) maps 1:1.  Shapes are the
 * reference's (OIHW conv weights, [out,in] linears). */
int dsx_model_num_params(const dsx_model* m);
int dsx_model_param_info(const dsx_model* m, int index, char* name_buf, int name_cap,
                         int* ndim, int64_t shape[4]);
/* Copies one parameter (fp32, reference layout, host memory). */
int dsx_model_set_param(dsx_model* m, int index, const float* host_data, int64_t numel);
/* sr3 only: the PositionalEncoding frequency table exp(-ln(1e4)*k/(d/2)),
 * k<d/2 (sr3 unet.py:24-28); optional — computed with expf() if never set. */
int dsx_model_set_posenc_freq(dsx_model* m, const float* host_freq, int count);
/* Repacks all weights into the kernels' layouts (MFMA fragment order, fp32 or
 * bf16) and uploads them to the current HIP device. */
int dsx_model_finalize(dsx_model* m, int compute_dtype);
/* Packed-weight cache: the repack of a checkpoint (model/model.py:153-166 loads `*_gen.pth`; the engine then
 * reorders every conv into MFMA fragment order) is done once.  dsx_model_export_packed copies the device image of
 * a finalized model to host memory (dsx_model_packed_bytes bytes for this model and dtype); dsx_model_finalize_packed
 * finalizes a freshly created model of the same configuration straight from such an image: no dsx_model_set_param,
 * no repacking.  The image layout depends on (configuration, dtype, DSX_ABI_VERSION): callers key their cache on
 * those and on the checkpoint's hash. */
int dsx_model_packed_bytes(dsx_model* m, int compute_dtype, size_t* bytes);
int dsx_model_export_packed(const dsx_model* m, void* host_buf, size_t capacity);
int dsx_model_finalize_packed(dsx_model* m, int compute_dtype, const void* host_image, size_t bytes);
/* Algorithmic FLOPs (2*MAC of conv/linear/attention contractions) of one
 * forward of one image of H x W. */
double dsx_model_flops(const dsx_model* m, int H, int W);

/* --------------------------------------------------------------- executor */

typedef struct dsx_exec dsx_exec;

/* Plans one UNet forward for a fixed (B,H,W): kernel list, tile shapes,
 * activation workspace (hipMalloc'ed once, sized for 288 GB parts: no reuse
 * games).  cond_channels > 0 declares that the first conv reads its input as
 * two tensors (cond, x) instead of a materialised torch.cat
 * (sr3 diffusion.py:157-158). */
int dsx_exec_create(dsx_model* m, int B, int H, int W, int cond_channels, dsx_exec** out);
void dsx_exec_destroy(dsx_exec* ex);
size_t dsx_exec_workspace_bytes(const dsx_exec* ex);
/* Diagnostics of the conv kernel's in-workgroup hand-off (bounded spins on LDS counters, tiles with three MFMA
 * images): how many spins gave up since dsx_exec_create.  0 in every correct run -- a non-zero count means pixels of
 * some launch were wrong and the caller must not use them.  Synchronises the device. */
int dsx_exec_handoff_timeouts(dsx_exec* ex, unsigned* count);
/* Host-only (no device needed): runs the planner's sizing pass and its planning pass for this geometry and
 * reports the workspace bytes each of them walked and the launch count.  The two must agree; dsx_exec_create
 * fails if they do not.  Lets CPU tests pin the planner under every tile-preference environment setting. */
int dsx_plan_dry_run(const dsx_unet_cfg* cfg, int compute_dtype, int B, int H, int W, int cond_channels,
                     size_t* sizing_bytes, size_t* planning_bytes, int* launches);
int dsx_exec_num_launches(const dsx_exec* ex);

/* Launch-level introspection for measurement (bench.py roofline): the plan's
 * launches in order, what each computes, and an eager hipEvent-timed replay. */
enum { DSX_OP_CONV_MFMA = 0, DSX_OP_CONV_NAIVE = 1, DSX_OP_GN_STATS = 2, DSX_OP_GN_FINALIZE = 3,
       DSX_OP_ATTN_GEMM = 4 /* the fused attention kernel */, DSX_OP_SOFTMAX = 5 /* unused since ABI 2 */,
       DSX_OP_SPLITK_REDUCE = 6 };
int dsx_exec_num_ops(const dsx_exec* ex);
int dsx_exec_op_info(const dsx_exec* ex, int index, char* desc_buf, int desc_cap, int* kind,
                     double* flops, double* bytes);
int dsx_exec_profile(dsx_exec* ex, int iters, float* ms_per_op, void* stream);
/* The launches of one kind (DSX_OP_*) captured into a hipGraph of their own and replayed `iters` times
 * between two hipEvents on `stream`: *ms_per_replay is the time of one back-to-back pass over them, i.e.
 * what `rocprofv3 --kernel-trace` sums for that kernel family inside the captured sampling step (the eager
 * per-launch times of dsx_exec_profile additionally contain the launch gaps). Inputs are whatever the
 * workspace holds; the timing of these kernels does not depend on the data. */
/* kind >= 0: that kind only; -1: every launch of the forward; <= -2: every launch except kind (-kind - 2), so that
 * time(-1) - time(-2 - k) is the time kind k takes INSIDE the forward (neighbouring launches warm its caches). */
int dsx_exec_time_kind(dsx_exec* ex, int kind, int iters, float* ms_per_replay, int* launches, void* stream);
/* diagnostics: in-kernel phase stamps (s_memtime) of the conv launch selected by DSX_STAMP_OP */
int dsx_exec_read_stamps(dsx_exec* ex, unsigned long long* out128);

/* Layer table (verification): what each layer of the plan reads and writes, recorded by the planning pass; the plan
 * itself is unaffected.  The workspace is never reused, so after one dsx_unet_forward every address below still holds
 * that forward's value and a test can recompute each layer from the kernels' own inputs.  Addresses are device
 * addresses inside the workspace (0 = absent); tensors are NHWC in their storage type (DSX_DTYPE_*) with row pitch
 * `*_ld` elements per pixel; per-channel vectors (gn_scale / gn_shift [B][C0 + C1], film [B][film_bs]) are fp32.
 *   CONV  : out = conv(act(cat(src0, src1))) + bias + film + resid; act = GroupNorm (gn_scale / gn_shift, or inside
 *           the kernel when gn_in_kernel) then Swish if `swish`; `up`: nearest x2 in front of the conv.
 *   ATTN  : out[B][L][C] (ld C) = softmax(q k^T / sqrt(C)) v, q / k / v rows of pitch `ld` (q = src0, k = src1,
 *           v = resid).
 *   FILM  : out = the [B][film_bs] FiLM vector of every ResnetBlock (conv1's bias folded in where bias_in_film).
 *   INPUT : out = channels [C0, C0 + Cout) of the network input, staged (B, Ho, Wo, Cout) in the storage type. */
enum { DSX_LAYER_CONV = 0, DSX_LAYER_ATTN = 1, DSX_LAYER_FILM = 2, DSX_LAYER_INPUT = 3 };
typedef struct dsx_layer_info {
  int32_t kind;                       /* DSX_LAYER_* */
  int32_t op_begin, op_end, op_main;  /* ops [op_begin, op_end) of dsx_exec_op_info compute it; op_main: its conv /
                                         attention launch */
  int32_t ks, stride, up, swish;
  int32_t B, Hs, Ws, Ho, Wo;
  int32_t C0, C1, src_dtype;          /* sources (attention: C0 = C1 = head dimension, L = Ho * Wo) */
  int32_t gn_gamma_param, gn_beta_param, gn_in_kernel;     /* -1: no GroupNorm */
  int32_t w_param, b_param, bias_in_film;                  /* dsx_model_param_info indices, -1: none */
  int32_t film_off, film_bs;                               /* film + film_off: this layer's [B] x Cout slice */
  int32_t resid_ld, out_ld, Cout, out_dtype, ld;           /* ld: attention q / k / v pitch */
  int32_t reserved;
  uint64_t src0, src1, gn_scale, gn_shift, film, resid, out;
} dsx_layer_info;
int dsx_exec_num_layers(const dsx_exec* ex);
int dsx_exec_layer_info(const dsx_exec* ex, int index, dsx_layer_info* info);
/* Copies `bytes` from device address `src` (which must lie inside the workspace) to the caller's device buffer `dst`
 * on `stream`. */
int dsx_exec_copy_workspace(const dsx_exec* ex, uint64_t src, size_t bytes, void* dst_dev, void* stream);

/* One UNet forward: replaces denoise_fn(x, t)
 * (sr3 unet.py:235-259 / ddpm unet.py:220-243).
 *   x_nchw_dev : (B, in_channel, H, W) fp32, NCHW as the reference passes it
 *   time_dev   : n_time fp32 values; n_time == B (sr3 gamma (B,1), ddpm t (B,))
 *                or 1 (InDI's single scalar, indi.py:65); NULL when
 *                with_time_emb == 0
 *   y_nchw_dev : (B, out_channel, H, W) fp32 */
int dsx_unet_forward(dsx_exec* ex, const float* x_nchw_dev, const float* time_dev, int n_time,
                     float* y_nchw_dev, void* stream);

/* TimePredictor head (time_predictor.py:35-44): relu(unet(x)) * sigmoid(conv7x7(x)),
 * masked mean per image.  mask_w: (1,in,7,7) host fp32, mask_b: (1,) host. */
int dsx_time_predictor_set_mask(dsx_exec* ex, const float* mask_w_host, const float* mask_b_host);
int dsx_time_predictor_forward(dsx_exec* ex, const float* x_nchw_dev, float* t_out_dev, void* stream);

/* ---------------------------------------------------------------- sampler */

/* One row per reverse step, in execution order (host-computed, fp32, so that
 * "schedule indexing" is bit-exact with the reference):
 *   tcond : value fed to the UNet's time embedding
 *           (sr3: sqrt_alphas_cumprod_prev[i+1], diffusion.py:153-154;
 *            ddpm: float(i); InDI: fp32(cur_t), indi.py:65)
 *   predict_eps = 1 (SR3/DDPM, diffusion.py:141-175):
 *           x0 = a*x - b*eps ; clamp(+-1) if clip ; x <- (c1*x0 + c2*x) + sigma*z
 *   predict_eps = 0 (InDI, indi.py:62-69):
 *           x <- (c1*net + c2*x) + sigma*z      (a, b ignored)
 * Every product and sum is rounded separately, like the reference's op
 * sequence (no FMA contraction). */
typedef struct dsx_step_table {
  int32_t n_steps;
  int32_t predict_eps;
  int32_t clip;
  const float* tcond;   /* host, n_steps */
  const float* a;
  const float* b;
  const float* c1;
  const float* c2;
  const float* sigma;
  /* 0: one row of scalars per step, shared by the batch (the reference's loops).  B (= the executor's batch): every
   * column holds n_steps * B values, [step][sample] — per-sample schedules, e.g. InDI started at a per-tile t
   * predicted by the TimePredictor (core/psnr_based_t_refinement.py:22-36 loops over the batch one sample at a time) */
  int32_t per_sample;
} dsx_step_table;

/* Runs the whole reverse loop on `stream` without host synchronisation:
 * replaces GaussianDiffusion.p_sample_loop (sr3 diffusion.py:177-203,
 * ddpm diffusion.py:205-237) and InDI.inference's loop (indi.py:86-90).
 *   cond_nchw_dev : (B, cond_channels, H, W) or NULL (must match dsx_exec_create)
 *   x_nchw_dev    : (B, C, H, W) in: initial state (the caller draws it, as
 *                   diffusion.py:194 / indi.py:82 do); out: final state, FULL batch
 *   noise_nchw_dev: NULL -> device Philox normals keyed by (seed, step);
 *                   else (n_steps, B, C, H, W) injected draws in the
 *                   reference's draw order (parity mode)
 *   snap_steps    : host array of step ordinals (0-based) after which the
 *                   state is copied to snap_nchw_dev[k] (B,C,H,W each); may be NULL
 *   use_graph     : 1 = capture one step into a hipGraph and replay it */
int dsx_sample_loop(dsx_exec* ex, const dsx_step_table* tab,
                    const float* cond_nchw_dev, float* x_nchw_dev,
                    const float* noise_nchw_dev, uint64_t seed,
                    const int32_t* snap_steps, int n_snap, float* snap_nchw_dev,
                    int use_graph, void* stream);

/* One reverse step on the state x (B, C, H, W) in place: dsx_sample_loop with a one-row table, eager.
 *   dsx_sr3_step : p_sample of sr3 / ddpm (sr3 diffusion.py:141-175): the step's scalars as set_new_noise_schedule
 *                  tabulates them -- noise_level = sqrt_alphas_cumprod_prev[t+1], sqrt_recip_alphas_cumprod[t],
 *                  sqrt_recipm1_alphas_cumprod[t], posterior_mean_coef1/2[t], sigma = exp(0.5 posterior_log_variance
 *                  _clipped[t]) (0 at t == 0: no draw)
 *   dsx_indi_step: inference_one_step of InDI (indi.py:62-69): x <- c_x0 UNet(x, t) + c_xt x + noise_scale z with
 *                  c_x0 = delta / t, c_xt = 1 - delta / t, noise_scale = e (t - delta)
 * noise_dev: (1, B, C, H, W) injected draw or NULL -> Philox normals keyed by seed. */
int dsx_sr3_step(dsx_exec* ex, float noise_level, float sqrt_recip_alphas_cumprod, float sqrt_recipm1_alphas_cumprod,
                 float posterior_mean_coef1, float posterior_mean_coef2, float sigma, int clip_denoised,
                 const float* cond_nchw_dev, float* x_nchw_dev, const float* noise_dev, uint64_t seed, void* stream);
int dsx_indi_step(dsx_exec* ex, float t_cur, float c_x0, float c_xt, float noise_scale, float* x_nchw_dev,
                  const float* noise_dev, uint64_t seed, void* stream);

/* Fills n fp32 values with N(0,1) from the engine's Philox4x32-10 stream. */
int dsx_randn(float* out_dev, int64_t n, uint64_t seed, uint64_t subsequence, void* stream);

/* -------------------------------------------------------------- objective
 * The forward half of the training objective (p_losses): one noising launch, one UNet forward (dsx_unet_forward, with
 * per-sample time values), one reduction.  No gradients anywhere.
 *
 * dsx_q_sample: q_sample of the three sampler families (sr3 diffusion.py:215-222, ddpm diffusion.py:266-274,
 * indi.py:116-124) in one launch, NCHW fp32, per element
 *   xe == NULL :  dst = c0[b]*x0 + c2[b]*z
 *   else       :  dst = (c0[b]*x0 + c1[b]*xe) + c2[b]*z
 * with every product and sum rounded separately (no FMA contraction), as the step table above.  The two-term form
 * adds no zero term.  c0 / c1 / c2: device arrays of B values (c1 may be NULL iff xe is).
 *   x0  : (B, C, H, W)
 *   xe  : (B, Ce, H, W), C % Ce == 0, read at channel c % Ce: cat([input] * out_channel, 1) of indi.py:157 without
 *         materialising it
 *   dst : (B, Cdst, H, W), written at channels coff .. coff + C - 1 (coff + C <= Cdst), the others left untouched: a
 *         conditional model's UNet input cat([input, x_noisy], 1) needs no second pass
 *   z   : (B, C, H, W) injected draws; NULL -> the Philox normals dsx_randn writes for (seed, subsequence) at the
 *         same flat index, bitwise, also stored to z_out (B, C, H, W) when that is not NULL (the Gaussian loss is
 *         taken against them).  z_out is ignored when z is given.
 * 16-byte accesses when H*W is a multiple of 4 and the pointers are 16-byte aligned, a scalar path otherwise.
 *
 * dsx_loss: per sample, sum |a - b| (squared == 0: nn.L1Loss) or sum (a - b)^2 (nn.MSELoss) over (C, H, W) of
 * a, b (B, C, H, W) fp32: difference, square and accumulation in double over a fixed partition
 * (dsx_loss_blocks(C, H, W) workgroups per sample, a function of the shape only) with a fixed-order finish, no
 * atomics: equal inputs give bitwise-equal outputs.  partial_dev holds B * dsx_loss_blocks doubles, per_sample_dev
 * receives B doubles (device; nothing is synchronised).  The caller applies the reduction (sum or mean). */
int dsx_q_sample(const float* x0_dev, const float* xe_dev, int B, int C, int Ce, int H, int W,
                 const float* c0_dev, const float* c1_dev, const float* c2_dev,
                 const float* z_dev, uint64_t seed, uint64_t subsequence, float* z_out_dev,
                 float* dst_dev, int Cdst, int coff, void* stream);
int dsx_loss_blocks(int C, int H, int W);
int dsx_loss(const float* a_dev, const float* b_dev, int B, int C, int H, int W, int squared,
             double* partial_dev, double* per_sample_dev, void* stream);

/* --------------------------------------------------------------- attention
 * dsx_attention: the UNet's fused single-head self-attention on caller tensors, exactly the launch the planner makes:
 *   out[b][i][0..C) = sum_j softmax_j(q_i . k_j / sqrtf(C)) v_j     per image b, over that image's L tokens
 * qkv_dev holds B * L token rows of ld elements; q, k and v are the column ranges [q_col, q_col + C), [k_col, ..),
 * [v_col, ..) of the same rows.  One buffer, because the kernel reads all three through one buffer descriptor per
 * image: based at q's first row of the image, L * ld * ES bytes long (ES: element size), which is what keeps rows past
 * L and columns past C out of the result without a branch.  Hence k_col >= q_col and v_col >= q_col (offsets are
 * taken relative to q), every range inside the row, and L * ld * ES < 2^31.
 *   storage  : element type of qkv and out: 0 fp32, 1 bf16, 2 fp16 (DSX_DTYPE_*)
 *   out_dev  : B * L rows of ldo elements (ldo >= C, ldo % 4 == 0); columns >= C are left untouched
 *   col_split: 0 / 1, the planner's attn_cs knob: with 257..512 channels and at most 160 query tiles of 32 rows, two
 *              workgroups share a tile, half of the output channels each
 * C in 8..1024 and a multiple of 8; column offsets and ld multiples of the 16-byte unit (4 fp32 / 8 16-bit elements);
 * both base pointers 16-byte aligned.  Anything else is refused with DSX_ERR_INVALID before any device work.  One
 * launch on `stream`, nothing allocated or synchronised. */
int dsx_attention(const void* qkv_dev, int ld, int q_col, int k_col, int v_col, void* out_dev, int ldo, int storage,
                  int B, int L, int C, int col_split, void* stream);

/* ------------------------------------------------------- validation report
 * dsx_val_report: what the training loop's validation block computes per item (split.py:174-241) on the NCHW fp32
 * visuals input (B, Cin, H, W), target and prediction (B, C, H, W), C <= DSX_VAL_MAX_CHANNELS, B * (C + Cin) <= 65535.
 * Two launches on `stream`, nothing allocated or synchronised; the second reads the first's partial statistics.
 *
 * Launch 1, in double with every product and sum rounded separately (numpy: a float32 array against float64 scalars),
 * the casts truncating:
 *   input_q  = uint16((input * std_input + mean_input) / 2)
 *   target_q = uint16(target * std_target[c] + mean_target[c])
 *   pred_q   = uint16(clip(prediction * std_target[c] + mean_target[c], 0, 65535))
 * A value that is NaN before its cast, and a target or input value outside [0, 65536), has no defined uint16 (the
 * reference's cast is undefined behaviour there): it is stored as 0 and counted.  Each workgroup owns DSX_VAL_CHUNK
 * pixels of one plane and writes one row of four words {sum (target_q - pred_q)^2, min, max, undefined pixels} to
 * partial_dev: 4 * DSX_VAL_PART_ROWS(B, Cin, C, H, W) uint64_t.  All statistics are integers: exact, and independent of
 * the reduction order.
 *
 * Launch 2 writes stats_dev, DSX_VAL_STATS_WORDS(B, Cin, C) uint64_t:
 *   [0]                            undefined pixels, all planes
 *   [1 + 3 (b C + c) + {0,1,2}]    sum (target_q - pred_q)^2, min and max of target_q over plane (b, c)
 *   [1 + 3 B C + 2 (b Cin + i) + {0,1}]   min and max of input_q over plane (b, i)
 * and, when the three numerator arrays are given (all or none; same shapes as the *_q arrays), the numerators of the
 * [0, 1] images the block writes in 'L' mode:
 *   target_n = target_q - tmin,   input_n = input_q - (min over the item's input planes),
 *   pred_n   = min((pred_q - tmin) mod 2^16, tmax - tmin)
 * the reference's uint16 subtraction wraps where the prediction lies below the target's minimum and its clip to 1 then
 * saturates the pixel; the denominators are tmax - tmin and imax - (item minimum).
 *
 * mean_target / std_target: host arrays of C doubles.  16-byte loads and 8-byte stores when H*W is a multiple of 4,
 * the fp32 pointers are 16-byte and the uint16 pointers 8-byte aligned; a scalar path otherwise. */
#define DSX_VAL_CHUNK 4096
#define DSX_VAL_MAX_CHANNELS 16
#define DSX_VAL_PART_ROWS(B, Cin, C, H, W) \
  ((size_t)(B) * ((size_t)(C) + (size_t)(Cin)) * (((size_t)(H) * (size_t)(W) + DSX_VAL_CHUNK - 1) / DSX_VAL_CHUNK))
#define DSX_VAL_STATS_WORDS(B, Cin, C) (1 + (size_t)(B) * (3 * (size_t)(C) + 2 * (size_t)(Cin)))
int dsx_val_report(const float* input_dev, const float* target_dev, const float* prediction_dev,
                   int B, int Cin, int C, int H, int W, double mean_input, double std_input,
                   const double* mean_target, const double* std_target,
                   uint16_t* input_q_dev, uint16_t* target_q_dev, uint16_t* pred_q_dev,
                   uint16_t* input_n_dev, uint16_t* target_n_dev, uint16_t* pred_n_dev,
                   uint64_t* partial_dev, uint64_t* stats_dev, void* stream);

/* ------------------------------------------------- caller-driven reverse sampling
 * The single reverse steps of the sampler classes as the caller's own loop uses them (p_mean_variance / p_sample, sr3
 * diffusion.py:151-175, ddpm diffusion.py:179-203; inference_one_step, indi.py:62-69) and the start of interpolate
 * (ddpm diffusion.py:249-259).  The UNet forward in front of a step is dsx_unet_forward.  NCHW fp32 device tensors, one
 * launch each, nothing allocated or synchronised; every product and sum rounded separately (no FMA contraction);
 * 16-byte accesses when H*W is a multiple of 4 and the pointers are 16-byte aligned, a scalar path otherwise.
 *
 * dsx_posterior_step: the update of dsx_step_table with per-sample coefficients (device arrays of B values each) and
 * its intermediate quantities, per element of sample b
 *   x0   = a[b]*x - b[b]*net, clamped to +-1 if clip    (predict_eps == 0: x0 = net, never clamped; a, b may be NULL)
 *   mean = c1[b]*x0 + c2[b]*x
 *   out  = mean + z*sigma[b]                             (sigma[b] == 0: out = mean, nothing drawn, nothing added)
 *   x, net : (B, C, H, W)
 *   z      : (B, C, H, W) injected draws, or NULL -> the Philox normals dsx_randn writes for (seed, subsequence) at the
 *            same flat index, bitwise.  repeat_noise != 0: every sample takes the draw of sample 0 (noise_like(...,
 *            repeat=True), ddpm diffusion.py:70-75); an injected z then holds (1, C, H, W).  Read only for x_out.
 *   x_recon_out, mean_out, x_out : (B, C, H, W) each, any of them NULL (not all three), those are left untouched;
 *            x_out may be x (in place).
 *
 * dsx_interp_start:  out = c*(a0[b]*x1 + s0[b]*z1) + d*(a0[b]*x2 + s0[b]*z2), the two inner expressions being
 * dsx_q_sample's two-term form bitwise; c = (float)(1 - lam), d = (float)lam.  z1, z2 (B, C, H, W): both injected, or
 * both NULL -> the Philox streams (seed, subsequence) and (seed, subsequence + 1), in that order. */
int dsx_posterior_step(const float* x_dev, const float* net_dev, int B, int C, int H, int W,
                       const float* a_dev, const float* b_dev, const float* c1_dev, const float* c2_dev,
                       const float* sigma_dev, int predict_eps, int clip,
                       const float* z_dev, uint64_t seed, uint64_t subsequence, int repeat_noise,
                       float* x_recon_out_dev, float* mean_out_dev, float* x_out_dev, void* stream);
int dsx_interp_start(const float* x1_dev, const float* x2_dev, int B, int C, int H, int W,
                     const float* a0_dev, const float* s0_dev, float c, float d,
                     const float* z1_dev, const float* z2_dev, uint64_t seed, uint64_t subsequence,
                     float* out_dev, void* stream);

/* ------------------------------------------------------- per-sample noise streams
 * An opt-in second way of drawing, for sampling that does not depend on how the work is batched or sharded: every
 * sample owns the streams named by (seed, sample id), and a draw is a pure function of
 *   (seed, sample id, draw ordinal, element index j inside the sample's (C, H, W) tensor in NCHW order)
 * -- not of B, of the sample's position in the batch, of the storage layout or of the rank.
 *
 * Definition, through the generator above: the sample stream (seed, id, draw) IS the stream
 *   (seed, subsequence = (id << 24) | draw)
 * of dsx_randn, and element j of the sample is element j of that stream (component j % 4 of Philox block j / 4).
 * id < 2^40 (DSX_STREAM_ID_LIMIT) and draw < 2^24 (DSX_STREAM_DRAW_LIMIT); anything else is refused.
 * Draw ordinal 0 is the initial state of a loop; ordinal s + 1 belongs to step s (0-based, execution order) of it.  A
 * step that adds no noise (sigma == 0: SR3's and InDI's last step) draws nothing and still owns its ordinal.
 *
 * dsx_randn_samples: out (B, chw) fp32, row b = the first chw elements of the stream (seed, ids[b], draw): what
 * dsx_randn(out + b * chw, chw, seed, (ids[b] << 24) | draw) writes, bitwise.  16-byte stores when chw is a multiple
 * of 4 and out is 16-byte aligned, scalar stores (with the tail of the last block) otherwise.  ids_host: B host values,
 * read before the call returns.
 *
 * dsx_sample_loop_streams: dsx_sample_loop with device noise drawn from the sample streams: step s of sample b adds
 * sigma * element (c * H * W + hw) of the stream (seed, sample_ids[b], s + 1) at state element (b, c, hw), whatever
 * the layout of the state inside the loop.  The caller draws the initial state (draw 0, dsx_randn_samples).  The ids
 * are copied to device memory the executor owns before the loop starts; a captured step graph reads them from there,
 * so one kept graph serves every call whatever its ids.  n_sample_ids must equal the executor's B; n_steps <
 * DSX_STREAM_DRAW_LIMIT; injected noise together with ids is refused (noise_nchw_dev must be NULL).  With the same
 * draws injected -- noise[s][b] = dsx_randn_samples(.., ids, s + 1) -- dsx_sample_loop computes the same bits.
 *
 * dsx_posterior_step_streams: dsx_posterior_step with z = the sample streams (seed, sample_ids[b], draw), `draw` taking
 * the place of `subsequence`; an injected z_dev and repeat_noise are refused (a shared draw is what streams are not),
 * n_sample_ids must equal B.  A caller-driven loop of dsx_unet_forward and this call with draw = s + 1 at step s
 * reproduces dsx_sample_loop_streams bit for bit. */
#define DSX_STREAM_ID_LIMIT ((uint64_t)1 << 40)
#define DSX_STREAM_DRAW_LIMIT ((uint32_t)1 << 24)
int dsx_randn_samples(float* out_dev, int B, int64_t chw, uint64_t seed, const uint64_t* ids_host, uint32_t draw,
                      void* stream);
int dsx_sample_loop_streams(dsx_exec* ex, const dsx_step_table* tab,
                            const float* cond_nchw_dev, float* x_nchw_dev,
                            const float* noise_nchw_dev, uint64_t seed,
                            const int32_t* snap_steps, int n_snap, float* snap_nchw_dev,
                            int use_graph, void* stream,
                            const uint64_t* sample_ids_host, int n_sample_ids);
int dsx_posterior_step_streams(const float* x_dev, const float* net_dev, int B, int C, int H, int W,
                               const float* a_dev, const float* b_dev, const float* c1_dev, const float* c2_dev,
                               const float* sigma_dev, int predict_eps, int clip,
                               const float* z_dev, uint64_t seed, uint64_t draw, int repeat_noise,
                               float* x_recon_out_dev, float* mean_out_dev, float* x_out_dev, void* stream,
                               const uint64_t* sample_ids_host, int n_sample_ids);

/* ------------------------------------------------------- few-step solvers (additive under DSX_ABI_VERSION 2)
 * DDIM and DPM-Solver++(2M, data prediction) over a sub-sequence of the trained schedule.  The host builds one row per
 * step (diffsplitting_amd/model/solvers.py, float64 rounded to fp32 once); the device evaluates, every product and sum
 * rounded separately,
 *   x0  = a*x - b*eps, clamped to +-1 if clip            (dsx_step_table's expression with predict_eps = 1)
 *   m   = c0*x0 + cx*x
 *   m   = cp != 0 ? m + cp*x0_prev : m                   (x0_prev: the x0 of the previous step; not read when cp == 0)
 *   x  <- m + sigma*z                                    (noise rules as in dsx_sample_loop / dsx_posterior_step)
 * This is the update of dsx_step_table with one more term, and the device states it once: a row of dsx_step_table is
 * the solver row (c0 = c1, cx = c2 -- mind the column order here: cx, then c0) with cp == 0, bit for bit, so DDIM rows
 * through dsx_solver_loop and through dsx_sample_loop give the same bits.
 *
 * dsx_solver_loop: dsx_sample_loop over such rows, through the same update kernel.  The previous x0 lives in a device buffer the executor allocates at
 * the first call and keeps (outside the workspace: dsx_exec_workspace_bytes does not change); the captured step differs
 * from the ancestral one, and an executor that alternates between the two loops recaptures.  cp[0] must be 0 (no
 * previous x0 at the first step).  sample_ids_host == NULL: the default noise (noise_nchw_dev or Philox (seed, step + 1));
 * else B ids of the per-sample noise streams, as in dsx_sample_loop_streams.
 *
 * dsx_solver_step: one update on NCHW tensors with per-sample coefficients (device arrays of B values each):
 * dsx_posterior_step's kernel with predict_eps = 1 and the history term.  x0_prev_dev: (B, C, H, W), read only for the samples whose cp != 0, or NULL
 * (every cp then counts as 0; cp_dev may be NULL too).  x_recon_out_dev receives x0 -- the next call's x0_prev_dev, it
 * may be the very buffer -- and x_out_dev the new state (it may be x_dev); both are required.  z_dev: injected draws or
 * NULL -> the stream (seed, subsequence); with sample_ids_host the sample streams (seed, sample_ids[b], draw) and z_dev
 * must be NULL.  A caller-driven chain of dsx_unet_forward and this call reproduces dsx_solver_loop bit for bit. */
typedef struct dsx_solver_table {
  int32_t n_steps;
  int32_t clip;
  const float* tcond;   /* host, n_steps each */
  const float* a;
  const float* b;
  const float* cx;
  const float* c0;
  const float* cp;
  const float* sigma;
} dsx_solver_table;
int dsx_solver_loop(dsx_exec* ex, const dsx_solver_table* tab,
                    const float* cond_nchw_dev, float* x_nchw_dev,
                    const float* noise_nchw_dev, uint64_t seed,
                    const int32_t* snap_steps, int n_snap, float* snap_nchw_dev,
                    int use_graph, void* stream,
                    const uint64_t* sample_ids_host, int n_sample_ids);
int dsx_solver_step(const float* x_dev, const float* net_dev, const float* x0_prev_dev, int B, int C, int H, int W,
                    const float* a_dev, const float* b_dev, const float* cx_dev, const float* c0_dev,
                    const float* cp_dev, const float* sigma_dev, int clip,
                    const float* z_dev, uint64_t seed, uint64_t subsequence,
                    float* x_recon_out_dev, float* x_out_dev, void* stream,
                    const uint64_t* sample_ids_host, int n_sample_ids, uint32_t draw);

/* ----------------------------------------------------------------- tiling */

enum { DSX_TILING_TRIM = 0, DSX_TILING_PAD = 1, DSX_TILING_SHIFT = 2 };  /* tiling_manager.py:6-12 */

/* Tile enumeration for data (N,H,W), replaces TileIndexManager
 * (data/tiling_manager.py:34-154) as SplitDatasetTiledPred sets it up
 * (data/split_dataset_tiledpred.py:9-24).  Host-only integer math.
 * Returns the tile count; if grid_start/patch_start are non-NULL they
 * receive count*3 entries (n, y, x). */
int64_t dsx_tile_plan(const int64_t data_shape[3], const int64_t grid_shape[3],
                      const int64_t patch_shape[3], int tiling_mode,
                      int64_t* grid_start, int64_t* patch_start, int64_t capacity);

/* Valid region of every tile (tile_stitcher.py:26-56): dst start (n,y,x),
 * extent (1,h,w) and the offset (y,x) inside the tile.  8 int32 per tile:
 * {n, y, x, h, w, ry, rx, 0}. */
int dsx_tile_regions(const int64_t data_shape[3], const int64_t grid_shape[3],
                     const int64_t patch_shape[3], int tiling_mode,
                     int32_t* regions, int64_t capacity);

/* Cuts tiles out of frames on the device: frames (N,H,W) fp32 ->
 * tiles (count, ph, pw) for the tiles listed in tile_ids (host array).
 * Replaces the per-item crop of SplitDataset.__getitem__
 * (data/split_dataset.py:237-246) for batch dispatch.
 * This and every other per-call form below (dsx_tiles_gather_*, dsx_stitch*) checks on the host, before anything
 * touches the device: count in 0..65535 (the tiles of a call are one launch), no negative id, every (frame, y, x) on
 * its int64 value inside the frames.  DSX_ERR_INVALID otherwise; count == 0 does nothing. */
int dsx_tiles_gather(const float* frames_dev, const int64_t data_shape[3],
                     const int64_t patch_shape[3], const int64_t* patch_start_host,
                     const int64_t* tile_ids_host, int64_t count, float* tiles_dev, void* stream);

/* dsx_tiles_gather for both raw channels plus the dataset's normalisation, fused: replaces
 * SplitDataset.__getitem__ (data/split_dataset.py:237-278: crop, normalize_target :199-201, weighted input,
 * normalize_inp :195-197) for a whole batch of tiles.  norm = {mean_input, std_input, mean_target0, std_target0,
 * mean_target1, std_target1} (float64, as compute_normalization_dict :29-74 returns them); from_norm_target selects
 * input = w0*target0 + w1*target1 (input_from_normalized_target).  tiles_in (count,1,ph,pw), tiles_target (count,2,ph,pw). */
int dsx_tiles_gather_norm(const float* frames0_dev, const float* frames1_dev, const int64_t data_shape[3],
                          const int64_t patch_shape[3], const int64_t* patch_start_host, const int64_t* tile_ids_host,
                          int64_t count, float w0, float w1, const double norm[6], int from_norm_target,
                          float* tiles_in_dev, float* tiles_target_dev, void* stream);

/* dsx_tiles_gather_norm for frames with colour planes: SplitDataset.__getitem__ on data_type 'cifar10'
 * (data/split_dataset.py:248-249 crop img[..., y:y+p, x:x+p] of (Cc, H, W) images, :265-266 concatenate + normalize_target
 * against the (2 Cc, 1, 1) statistics, :271-272 weighted input + normalize_inp), for a whole batch of items in one launch.
 * frames0/1 (N, Cc, H, W) fp32 with data_shape = {N, Cc, H, W}, 1 <= Cc <= 8; patch_hw = {ph, pw}; patch_start_host
 * holds (frame, y, x) triples and tile_ids_host selects from it (NULL: the first `count` triples), as for
 * dsx_tiles_gather_norm.  mean_target / std_target: 2 Cc doubles each, plane c of frames0 is target channel c, plane c
 * of frames1 is channel Cc + c.  Per element, every operation rounded on its own (no fma):
 *   target_c = (float)(((double)p_c - mean_target[c]) / std_target[c])
 *   input_c  = (float)(((double)fadd(fmul(w0, p0_c), fmul(w1, p1_c)) - mean_input) / std_input)
 * tiles_in (count, Cc, ph, pw), tiles_target (count, 2 Cc, ph, pw); nothing outside them is written.  count <= 65535
 * per call (larger batches are the caller's to slice).  DSX_ERR_INVALID with a message, before any device work: a NULL
 * pointer, Cc outside 1..8, a patch larger than the frame, a location outside the frame, a non-finite statistic or a
 * zero std, count outside 0..65535. */
int dsx_tiles_gather_norm_planes(const float* frames0_dev, const float* frames1_dev, const int64_t data_shape[4],
                                 const int64_t patch_hw[2], const int64_t* patch_start_host, const int64_t* tile_ids_host,
                                 int64_t count, float w0, float w1, double mean_input, double std_input,
                                 const double* mean_target, const double* std_target, float* tiles_in_dev,
                                 float* tiles_target_dev, void* stream);

/* The mixed inputs of the TimePredictor evaluation for a whole batch of tiles, from the two raw frame stacks, in one
 * pass: replaces get_inputs + normalize_indi1/2 (notebooks/EvaluateJointIndiIterative.ipynb cells 40, 43), the
 * classifier sweep's mixing (notebooks/time_prediction_evaluation.ipynb cell 4) and the arithmetic of
 * TimePredictorDataset.__getitem__ (data/time_predictor_dataset.py:50-89).  norm = {mean_target0, std_target0,
 * mean_target1, std_target1} (float64), t = the mixing weight of the call.  Outputs, each (count, 2, ph, pw) fp32,
 * any of them may be NULL (not all three):
 *   target : t0, t1 = the normalised channels, exactly as dsx_tiles_gather_norm writes them
 *   mix    : channel 0 = t0*(1-t) + t1*t (input of indi1), channel 1 = t1*(1-t) + t0*t (input of indi2)
 *   cls    : 2*(m - lo)/(hi - lo) - 1 of the two mix channels, lohi = {lo0, hi0, lo1, hi1}: the rows int((1-t)*n) and
 *            int(t*n) of the dsx_mix_range table (the caller picks the rows; lohi may be NULL iff cls is)
 * fp32, every operation rounded on its own (no fma), in this order:
 *   w1 = (float)t,  w0 = (float)(1.0 - t)                      (the subtraction in double)
 *   m0 = fadd(fmul(t0, w0), fmul(t1, w1)),  m1 = fadd(fmul(t1, w0), fmul(t0, w1))
 *   cls_c = fsub(fdiv(fmul(2, fsub(m_c, (float)lo_c)), (float)(hi_c - lo_c)), 1)   (hi - lo in double, IEEE division)
 * which is what torch computes for a float32 tensor and Python / float64 scalars.  TimePredictorDataset mixes
 * t*patch1 + (1-t)*patch2 and normalises with row t_int: channel 1.  Host-side refusals (before any device work):
 * all outputs NULL, non-finite t or statistics, zero std, cls with a non-finite or empty (hi == lo) row. */
int dsx_tiles_gather_mix(const float* frames0_dev, const float* frames1_dev, const int64_t data_shape[3],
                         const int64_t patch_shape[3], const int64_t* patch_start_host, const int64_t* tile_ids_host,
                         int64_t count, const double norm[4], double t, const double lohi[4], float* target_dev,
                         float* mix_dev, float* cls_dev, void* stream);

/* dsx_tiles_gather_mix for a batch whose items each carry their own mixing weight and table rows, in ONE launch: what
 * the TimePredictor's validation loop feeds the network (time_prediction_training.py:133-140, every item of
 * TimePredictorDataset draws its own t).  Item k is cut at patch_start_host[k] = (frame, y, x), mixed with t_host[k]
 * and, for cls, min-max-normalised with lohi_host[k] = {lo0, hi0, lo1, hi1}; lohi_host may be NULL iff cls_dev is.
 * Outputs as dsx_tiles_gather_mix: target / mix / cls, each (count, 2, ph, pw) fp32, any of them NULL (not all three);
 * nothing outside them is written.  The arithmetic per item is the chain documented there, unchanged (fp32, every
 * operation rounded on its own, no fma; 1.0 - t and hi - lo in double): item k is bitwise what dsx_tiles_gather_mix
 * writes for that location with t_host[k] and lohi_host[k].  The per-item scalars travel with the patch-start table
 * the call uploads (one allocation, one copy, one launch).  DSX_ERR_INVALID with a message that names the item, before
 * any device work: a NULL pointer, a non-finite t[k] or statistic, a zero std, a non-finite or empty (hi == lo) row, a
 * location outside the frame, count outside 0..65535. */
int dsx_tiles_gather_mix_items(const float* frames0_dev, const float* frames1_dev, const int64_t data_shape[3],
                               const int64_t patch_shape[3], const int64_t* patch_start_host, int64_t count,
                               const double norm[4], const double* t_host, const double* lohi_host, float* target_dev,
                               float* mix_dev, float* cls_dev, void* stream);

/* The range table the classifier's inputs are normalised with (compute_input_normalization_dict,
 * data/time_predictor_dataset.py:6-21), in one launch instead of n + 1 host passes over the frame set: for every
 * t_int in 0..n_timesteps the min and max over all `pixels` of both stacks (all frames, flat) of
 *   v = t*a + (1.0 - t)*b,   a = ((double)x0 - mean0)/std0,  b = ((double)x1 - mean1)/std1,  t = (double)t_int/n
 * in fp64 with every product, sum and quotient rounded on its own (never an fma): bitwise numpy's float64 result for
 * frames that fp32 holds exactly, bitwise repeatable (min / max do not depend on the reduction order).  Frames are
 * assumed finite.  norm = {mean0, std0, mean1, std1}; 1 <= n_timesteps <= 1024; non-finite statistics and zero std
 * are refused.  dsx_mix_range_blocks: rows of partials a call needs; partials_dev holds rows * (n_timesteps + 1) * 2
 * doubles.  out_minmax_host[(n_timesteps + 1)][2] = {min, max} is written after the stream is synchronised. */
int dsx_mix_range_blocks(int64_t pixels, int n_timesteps);
int dsx_mix_range(const float* frames0_dev, const float* frames1_dev, int64_t pixels, const double norm[4],
                  int n_timesteps, double* partials_dev, double* out_minmax_host, void* stream);

/* Pastes the valid region of `count` predicted tiles (count, C, ph, pw) into
 * the zero-initialised canvas (N,H,W,C), channel-last: replaces
 * stitch_predictions (data/tile_stitcher.py:10-81).  regions as from
 * dsx_tile_regions for exactly these tiles. */
int dsx_stitch(const float* tiles_dev, int64_t count, int C, int ph, int pw,
               const int32_t* regions_host, float* canvas_dev, const int64_t data_shape[3],
               void* stream);

/* dsx_stitch plus, in the same pass over the tiles, the sums the reported quality metric needs
 * (RangeInvariantPsnr, core/psnr.py:70-82) of the pasted prediction p against the ground-truth canvas g
 * (N,H,W,C fp32): partials_dev receives count * dsx_stitch_psnr_blocks(ph,pw) * C * 8 doubles
 * {sum p, sum p^2, sum g, sum g^2, sum g p, min g, max g, 0} per (tile, workgroup, channel); the caller adds the
 * rows of a frame (fixed order) and evaluates the closed form.  Replaces the host-side pass over the 335 MB
 * stitched canvas (notebooks/EvaluateJointIndi.ipynb cell 30). */
int dsx_stitch_psnr_blocks(int ph, int pw);
int dsx_stitch_psnr(const float* tiles_dev, int64_t count, int C, int ph, int pw, const int32_t* regions_host,
                    float* canvas_dev, const int64_t data_shape[3], const float* gt_canvas_dev, double* partials_dev,
                    void* stream);

/* Image-quality metrics of the reference's core/metrics.py on B image pairs a, b (B,C,H,W fp32 on the device), in one
 * pass: per image, the mean over its C channels of the SSIM map of ssim() (core/metrics.py:72-92: cv2.getGaussianKernel
 * (11, 1.5) window, valid region [5:-5, 5:-5], C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L = data_range, moments in fp64)
 * and the sum of squared differences over the whole image (calculate_psnr, :62-69).  quantize != 0 first maps both
 * images as tensor2img (:14-34) does: clamp to [lo, hi], (x - lo) / (hi - lo) in fp32, * 255, round half to even;
 * the SSD is then an exact integer.  H and W >= 11 (the reference returns NaN below).
 * dsx_image_metrics_blocks(H, W): workgroups per image plane; partials_dev holds B * C * blocks * 2 doubles.
 * out_ssim_host[B], out_ssd_host[B] (exact when quantised, below 2^53) are written after the stream is synchronised;
 * the per-block partials are added in a fixed order, so equal inputs give bitwise-equal outputs. */
int dsx_image_metrics_blocks(int H, int W);
int dsx_image_metrics(const float* a_dev, const float* b_dev, int B, int C, int H, int W, int quantize, double lo,
                      double hi, double data_range, double* partials_dev, double* out_ssim_host, double* out_ssd_host,
                      void* stream);

/* Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) of `planes` plane pairs (pred, target), each H x W fp32 on the
 * device, over `scales` scales (1..5); optionally range-invariant, for frames that have no natural peak.
 *   Window     the 11 taps of dsx_image_metrics (Gaussian, sigma 1.5), separable, valid region [5:-5, 5:-5] only;
 *              c1 = (0.01 L)^2, c2 = (0.03 L)^2, the same at every scale.
 *   Per scale  over the valid region, in double:  cs = (2 s12 + c2) / (s11 + s22 + c2),
 *              ssim = (2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1) * cs;  the means cs_s and ssim_s of both maps are the
 *              output, both at every scale: out_host[planes][scales][2] = {cs_s, ssim_s}.
 *   Between    2 x 2 mean pooling of both planes, an odd last row or column dropped (H -> H / 2):
 *              ((x00 + x01) + (x10 + x11)) * 0.25 in double; pooled planes stay double, never rounded to fp32.
 *   Result     prod_{s < S-1} max(cs_s, 0)^w_s * max(ssim_{S-1}, 0)^w_{S-1}, formed by the caller in double from the
 *              2 S means (core.metrics.msssim; Wang's weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333, not renormalised
 *              when fewer are used): the device owns the means only.
 *   Size rule  the coarsest scale still holds the window: min(H, W) >> (scales - 1) >= 11 (176 for five scales).
 *   range_invariant != 0 (data_range is then ignored): per plane the transform of RangeInvariantPsnr (core/psnr.py)
 *              in double, applied on the load of scale 0:  g' = (g - mean g) / std g (unbiased std),
 *              p' = alpha (p - mean p) with alpha = sum g' p~ / sum p~ p~, p~ = p - mean p, and L = (max g - min g) / std g.
 *              The plane statistics (sum g, g^2, p, p^2, g p; min and max of g and of p) come from one fixed-order double
 *              reduction on the device and the coefficients stay there.  std g == 0 or sum p~ p~ == 0 (recognised by
 *              min == max) gives NaN for that plane, not an error.  The value does not change under a positive affine
 *              map of the prediction or of the target, up to input rounding.
 * Everything is enqueued on `stream`, which is synchronised once, to read the planes * scales * 2 means.  The tile
 * partials are added in an order that depends on the shape alone and nothing uses atomics: equal inputs give
 * bitwise-equal outputs.  dsx_msssim_workspace(H, W, scales): bytes of workspace PER PLANE PAIR (negative: the shape
 * is refused); workspace_dev holds planes times that, 8-byte aligned, and every byte of it that the call reads the
 * call has written.  planes <= 65535. */
int64_t dsx_msssim_workspace(int H, int W, int scales);
int dsx_msssim(const float* pred_dev, const float* target_dev, int planes, int H, int W, int scales, int range_invariant,
               double data_range, void* workspace_dev, size_t workspace_bytes, double* out_host, void* stream);

/* ------------------------------------------------------------------ LPIPS
 * The perceptual metric of the reference's evaluation (notebooks/EvaluateJointIndi.ipynb cell 31 and
 * notebooks/EvaluateJointIndiIterative.ipynb cell 28: lpips.LPIPS(net='alex'), version 0.1, spatial off): scaling
 * layer, AlexNet feature trunk with its five ReLU taps, per tap the `lin`-weighted squared difference of the
 * unit-normalised features (f / (sqrt(sum_c f^2) + 1e-10)) averaged over space, summed over the taps.  fp32 on the
 * exact-fp32 matrix cores; the partial sums are added in a fixed order in double, so equal inputs give bitwise-equal
 * outputs.  Weights always come from the caller: nothing is ever fetched. */
typedef struct dsx_lpips dsx_lpips;
/* Restates LPIPS.__init__'s weight loading.  Host only (works without a GPU; the packed image is uploaded at first
 * use).  trunk_host: 10 fp32 host tensors in state_dict order, net.slice{1..5}.{0,3,6,8,10}.{weight,bias} (OIHW:
 * (64,3,11,11), (192,64,5,5), (384,192,3,3), (256,384,3,3), (256,256,3,3)); lin_host: lin{0..4}.model.1.weight
 * ((1,C,1,1), C = 64, 192, 384, 256, 256).  Element counts are checked and a mismatch is refused by key name. */
int dsx_lpips_create(const float* const* trunk_host, const int64_t* trunk_numel, const float* const* lin_host,
                     const int64_t* lin_numel, dsx_lpips** out);
void dsx_lpips_destroy(dsx_lpips* h);
/* Restates LPIPS.forward(in0, in1, normalize=False): in0 / in1 (B, 3, H, W) fp32 NCHW in [-1, 1] on the device ->
 * out_dev[B]; per_tap_dev (may be NULL) receives [B][5], the values retPerLayer=True returns.  Asynchronous on
 * `stream`.  H, W >= 31 (below that a stage of the trunk is empty); a batch whose largest tensor passes 2 GiB is
 * refused.  One workspace per handle and (B, H, W), reallocated when they change. */
int dsx_lpips_forward(dsx_lpips* h, const float* in0_nchw_dev, const float* in1_nchw_dev, int B, int H, int W,
                      float* out_dev, float* per_tap_dev, void* stream);
/* Restates compute_lpips of the notebooks for one channel of the stitched frames: target / pred (N, H, W, C) fp32
 * channel-last on the device; x -> 2 (x - min) / (max - min) - 1 in fp32 with min / max of the TARGET's channel over all
 * N frames (reduced on the device), replicated to three channels, one value per frame -> out_dev[N].  Frames go through
 * the trunk `chunk` at a time (0: as many as ~1.5 GiB of workspace hold); the values do not depend on it (bitwise).
 * A constant target channel divides by zero, as the reference does. */
int dsx_lpips_frames(dsx_lpips* h, const float* target_nhwc_dev, const float* pred_nhwc_dev, int N, int H, int W, int C,
                     int channel, int chunk, float* out_dev, void* stream);
/* Stage table (verification): the workspace keeps every stage of the last dsx_lpips_forward, so a test can recompute
 * each launch from that launch's own input.  Stages in order: x0 (the scaled input), f1 (conv1 + ReLU, tap 1), p1
 * (pool), f2 (conv2, tap 2), p2 (pool), f3, f4, f5 (conv3..5, taps 3..5); each is fp32 NHWC (nimg, H[s], W[s], C[s]) at
 * device address stage[s], image b of in0 first, then image b of in1 at nimg / 2 + b.  Per tap t: part[t] is the
 * address of [pairs][nblk[t]] doubles, the partial sums k_lpips_finish adds in order and divides by hw[t].  Read-only:
 * no launch, no result changes.  Refused before any forward and after dsx_lpips_frames, which reuses the workspace
 * per chunk. */
enum { DSX_LPIPS_STAGES = 8 };
typedef struct dsx_lpips_layer_table {
  int32_t pairs, nimg;
  int32_t H[DSX_LPIPS_STAGES], W[DSX_LPIPS_STAGES], C[DSX_LPIPS_STAGES];
  int32_t nblk[5], hw[5];
  uint64_t stage[DSX_LPIPS_STAGES];
  uint64_t part[5];
} dsx_lpips_layer_table;
int dsx_lpips_layers(const dsx_lpips* h, dsx_lpips_layer_table* table);
/* Copies `bytes` from device address `src` (which must lie inside the handle's workspace) to the caller's device
 * buffer `dst_dev` on `stream`. */
int dsx_lpips_copy_workspace(const dsx_lpips* h, uint64_t src, size_t bytes, void* dst_dev, void* stream);

/* ------------------------------------------------------------------ SR3 image path: resize and ToTensor
 * The first step of the reference's SR3 configurations (data/prepare_data.py:17-40 resize_and_convert /
 * resize_multiple, data/util.py:74-83 transform_augment): PIL's Image.resize on 8-bit images, antialiased BILINEAR or
 * BICUBIC (libImaging/Resample.c), and torchvision's ToTensor.  The resampler is fixed-point integer arithmetic --
 * int32 coefficients scaled by 2^22, per output sample ss = 2^21 + sum pixel * k over its tap window, output
 * clip(ss >> 22, 0, 255), horizontal pass first, uint8 between the passes, a pass that keeps the length skipped -- so
 * the device result equals PIL's byte for byte. */
enum { DSX_RESIZE_BILINEAR = 2, DSX_RESIZE_BICUBIC = 3 };   /* PIL.Image.BILINEAR / BICUBIC */
/* Restates precompute_coeffs + normalize_coeffs_8bpc for one axis.  Host only (works without a GPU).  Every
 * intermediate is a double rounded on its own, sums run in tap order: scale = in / out, filterscale = max(scale, 1),
 * support = {bilinear 1, bicubic 2} * filterscale; per output xx: center = (xx + 0.5) * scale, xmin = max(0,
 * (int)(center - support + 0.5)), xmax = min(in, (int)(center + support + 0.5)), weight x = filter((x + xmin -
 * center + 0.5) * (1 / filterscale)) (the product with the reciprocal, as Resample.c writes it), each row divided by
 * its sum, then (int)(+-0.5 + w * 2^22) with the sign of w.  Bicubic uses a = -0.5.  Returns the row capacity needed
 * (2 * ceil(support) + 1); with all three outputs NULL that is all it does, else xmin_out[out], n_out[out] (taps of
 * the row) and k_out[out][cap] (zero past the taps) are filled and cap must reach the capacity. */
int dsx_resize_coeffs(int in_size, int out_size, int filter, int32_t* xmin_out, int32_t* n_out, int32_t* k_out, int cap);
/* Image.resize((out_w, out_h), filter) of in_h x in_w images with C = 1 or 3 interleaved channels, followed by the
 * crop [crop_top, crop_top + crop_h) x [crop_left, crop_left + crop_w) of the resized image (center_crop of
 * resize_and_convert): only the window is computed.  The plan holds both coefficient tables (built here on the host,
 * uploaded once at first device use) and the tiling of the two passes.  Sizes below 1, another C or filter id, a window
 * that leaves the resized image and a resize whose single output does not fit the LDS staging (a reduction by several
 * thousand) are refused with DSX_ERR_INVALID. */
typedef struct dsx_resize_plan dsx_resize_plan;
int dsx_resize_plan_create(int in_h, int in_w, int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w,
                           int filter, int C, dsx_resize_plan** out);
void dsx_resize_plan_destroy(dsx_resize_plan* plan);
/* bytes of the uint8 intermediate between the passes for B images (0 when a pass is skipped) */
size_t dsx_resize_workspace_bytes(const dsx_resize_plan* plan, int B);
/* src_dev [B][in_h][in_w][C] uint8 -> dst_dev [B][crop_h][crop_w][C] uint8, asynchronous on `stream`; B <= 65535 */
int dsx_resize_u8(dsx_resize_plan* plan, const uint8_t* src_dev, int B, uint8_t* dst_dev, uint8_t* workspace_dev,
                  void* stream);
/* ToTensor and the min_max map of transform_augment: [B][H][W][C] uint8 -> [B][C][H][W] fp32, v = float(u) / 255.0f
 * (IEEE division), then v * (hi - lo) + lo with product and sum rounded separately: bitwise what torch computes on the
 * CPU for min_max = (lo, hi).  C = 1 or 3. */
int dsx_u8_to_tensor(const uint8_t* src_dev, int B, int H, int W, int C, float lo, float hi, float* dst_dev, void* stream);

/* ------------------------------------------------- tile plan with device-resident tables (the stall-free forms)
 * The entry points above take host tables and upload them per call (a small allocation and a synchronous copy each).
 * A dsx_tileplan keeps the patch starts and valid regions of every tile on the device (uploaded once, at first
 * device use); every call names its tiles as the arithmetic sequence first, first + stride, ... (count terms) -- the
 * shard r, r + W, r + 2W, ... of rank r, or a batch of it -- and the kernels index the tables by tile id: no
 * allocation, copy or synchronisation per call.  Replaces SplitDatasetTiledPred's per-index TileIndexManager lookups
 * (data/split_dataset_tiledpred.py:9-32) and stitch_predictions (data/tile_stitcher.py:10-81) for batch dispatch. */
typedef struct dsx_tileplan dsx_tileplan;
int dsx_tileplan_create(const int64_t data_shape[3], const int64_t grid_shape[3], const int64_t patch_shape[3],
                        int tiling_mode, dsx_tileplan** out);        /* host only; fails if a tile leaves the frames */
void dsx_tileplan_destroy(dsx_tileplan* plan);
int64_t dsx_tileplan_total(const dsx_tileplan* plan);
/* The plan's paste regions, 8 int32 per tile as dsx_tile_regions: stitch_predictions pastes tile after tile
 * (tile_stitcher.py:68-80), so where valid regions overlap (the shifted last tile of a ragged extent re-covers a strip
 * of its neighbour) the later tile's pixels stay; the plan clips the earlier tile's region to what survives, so that
 * all tiles can be pasted at once and every canvas pixel is written -- and exchanged -- exactly once. */
int dsx_tileplan_regions(const dsx_tileplan* plan, int32_t* regions, int64_t capacity);
/* dsx_tiles_gather / dsx_tiles_gather_norm for the tiles first + k*stride, k < count (<= 65535 per call) */
int dsx_tileplan_gather(dsx_tileplan* plan, const float* frames_dev, int64_t first, int64_t stride, int64_t count,
                        float* tiles_dev, void* stream);
int dsx_tileplan_gather_norm(dsx_tileplan* plan, const float* frames0_dev, const float* frames1_dev, int64_t first,
                             int64_t stride, int64_t count, float w0, float w1, const double norm[6],
                             int from_norm_target, float* tiles_in_dev, float* tiles_target_dev, void* stream);
/* dsx_tiles_gather_mix for the tiles of the sequence */
int dsx_tileplan_gather_mix(dsx_tileplan* plan, const float* frames0_dev, const float* frames1_dev, int64_t first,
                            int64_t stride, int64_t count, const double norm[4], double t, const double lohi[4],
                            float* target_dev, float* mix_dev, float* cls_dev, void* stream);
/* The network input of an INPUT-ONLY stack: frames_dev holds the plan's (N,H,W) frames in their file width, pix_type =
 * DSX_PIX_U8 / DSX_PIX_U16 / DSX_PIX_F32 (below; DSX_PIX_U32 is refused), in which the two structures are already
 * superimposed.  Per element of the tiles first + k*stride, k < count (1..65535 per call):
 *   x = (float)pixel (exact for the integer types);  upper_clip >= 0: x = min(x, (float)upper_clip);
 *   tiles_in = (float)(((double)x - mean_input) / std_input)
 * -- what dsx_tileplan_gather_norm (from_norm_target = 0) applies to w0 * p0 + w1 * p1: on a stack that holds
 * fl(fl(w0 * c0) + fl(w1 * c1)) the tiles equal that call's tiles_in bit for bit.  tiles_in_dev (count, 1, ph, pw).
 * Null pointers, another pixel type, a count outside 1..65535, tiles outside the plan, a non-finite mean and a
 * non-finite or non-positive std are DSX_ERR_INVALID before any HIP call. */
int dsx_tileplan_gather_input(dsx_tileplan* plan, const void* frames_dev, int pix_type, int64_t first, int64_t stride,
                              int64_t count, double mean_input, double std_input, double upper_clip,
                              float* tiles_in_dev, void* stream);
/* Frame-keyed noise for tiled prediction.  The NOISE FIELD (seed, id, draw) of a (C, H, W) frame is the sample stream of
 * dsx_randn_samples with that (seed, id, draw), read as a (C, H, W) tensor: element (c, y, x) is element
 * j = (c*H + y)*W + x of the stream (seed, (id << 24) | draw), i.e. component j % 4 of Philox block j / 4.  H and W
 * are the plan's frame extents.  out_dev (count, C, ph, pw) fp32: the tile first + k*stride, cut at patch start
 * (n, y0, x0), receives field(seed, id_base + n, draw)[c, y0 + yy, x0 + xx] -- the crop of what
 * dsx_randn_samples(.., C*H*W, seed, {id_base + n}, draw) writes, bit for bit.  Two tiles of one frame hold the same
 * bits wherever they overlap; a draw does not depend on the tile, the batch or the rank.  One 16-byte store per four
 * pixels when pw is a multiple of 4 and out_dev is 16-byte aligned, scalar stores otherwise.
 * A null plan, a sequence that leaves the plan and a count outside 0..65535 are refused as by the other plan forms
 * (count == 0: DSX_OK without a device); C < 1, id_base + (N - 1) >= DSX_STREAM_ID_LIMIT and
 * draw >= DSX_STREAM_DRAW_LIMIT are DSX_ERR_INVALID before any HIP call. */
int dsx_tileplan_randn(dsx_tileplan* plan, int C, int64_t first, int64_t stride, int64_t count, uint64_t seed,
                       uint64_t id_base, uint32_t draw, float* out_dev, void* stream);
/* Mean and spread over n repeated samples of `count` values (the posterior of a diffusion splitter), Welford's
 * recurrence in double, one launch per sample r = 0, 1, ... and one to finish:
 *   update, r == 0: mean = x, M2 = 0;  r > 0: d = x - mean;  mean' = mean + d / (r + 1);  M2' = M2 + d * (x - mean')
 *   finish: mean_out = (float)mean;  std_out = n > 1 ? (float)sqrt(M2 / (n - 1)) : 0      (std_out_dev may be NULL)
 * Every operation is rounded on its own (no fma): a float64 restatement of these lines in the same order is bit-equal.
 * r in 0..2^24 - 1, n in 1..2^24, count >= 1 and non-null pointers, or DSX_ERR_INVALID before any device work. */
int dsx_moments_update(const float* x_dev, double* mean_dev, double* m2_dev, int64_t count, int r, void* stream);
int dsx_moments_finish(const double* mean_dev, const double* m2_dev, int64_t count, int n, float* mean_out_dev,
                       float* std_out_dev, void* stream);
/* dsx_stitch (gt_canvas_dev == NULL) or dsx_stitch_psnr for whole predicted tiles (count, C, ph, pw) of the sequence */
int dsx_tileplan_stitch(dsx_tileplan* plan, const float* tiles_dev, int C, int64_t first, int64_t stride, int64_t count,
                        float* canvas_dev, const float* gt_canvas_dev, double* partials_dev, void* stream);
/* Multi-GPU exchange of CROPPED tiles (the crop of tile_stitcher.py:38-56 applied before the collective).
 * Rank q of `world` owns the tiles q, q + world, ...; its packed run holds their valid regions [C][h][w] back to back
 * in id order.  dsx_tileplan_pack_layout (host only) gives the pixel offset of every tile inside its rank's run and
 * the pixels of every rank's run (multiply by C for elements); the collective ships max(rank run) elements per rank
 * instead of whole (C, ph, pw) tiles.
 *   dsx_tileplan_pack        : tiles first, first + world, ... (count of them, (count, C, ph, pw)) -> their places in
 *                              flat_rank_dev, the run of rank first % world
 *   dsx_tileplan_paste_packed: every tile of the plan from the gathered buffer [world][rank_stride_elems] into the
 *                              canvas (N,H,W,C); with gt_canvas_dev also the PSNR partial sums (total * blocks * C * 8) */
int dsx_tileplan_pack_layout(const dsx_tileplan* plan, int world, int64_t* tile_offset_pixels /*[total]*/,
                             int64_t* rank_pixels /*[world]*/);
int dsx_tileplan_pack(dsx_tileplan* plan, const float* tiles_dev, int C, int world, int64_t first, int64_t count,
                      float* flat_rank_dev, void* stream);
int dsx_tileplan_paste_packed(dsx_tileplan* plan, const float* flat_all_dev, int C, int world, int64_t rank_stride_elems,
                              float* canvas_dev, const float* gt_canvas_dev, double* partials_dev, void* stream);
/* Blended stitching: the overlap-add of ALL predicted tiles of a plan into the canvas, instead of the paste of their
 * inner regions.  The plan's tiles must cover the frames with one frame per tile (SHIFT tiling of a (1, g, g) grid):
 * along an axis the patch starts are then 0, g, 2g, .., D - p, strictly increasing, so the tiles that cover a canvas
 * row (column) are one contiguous range of tile rows (columns).
 *   dsx_tileplan_contributors: host only; rows [H][2] = per canvas row (first tile row, count), cols [W][2] = per canvas
 *     column (first tile column, count).  Tile (iy, ix) of frame n has id (n*ny + iy)*nx + ix.
 *   dsx_tileplan_set_window: the separable window w(yy, xx) = wy[yy] * wx[xx] over a tile, wy_host [ph], wx_host [pw];
 *     host only.  Every value must be finite and > 0, or DSX_ERR_INVALID names the first that is not.  The window goes
 *     up once, at the next blend; a later call replaces it.
 *   dsx_tileplan_blend: tiles_dev holds every tile of the plan as whole (C, ph, pw) tiles -- world == 1: (total, C, ph,
 *     pw); world > 1: the gathered exchange buffer [world][rank_stride_elems], rank q's slot holding its tiles q,
 *     q + world, ... back to back (the sharding of dsx_tileplan_pack_layout, with whole tiles).  Per canvas pixel and
 *     channel, fp32, every operation rounded on its own (no fma), the division correctly rounded, the contributors in
 *     ASCENDING TILE ID:
 *         one contributor:  out = v                                   (a copy: the bits do not change)
 *         else  num = 0; den = 0;  per contributor:  w = wy[yy] * wx[xx];  num = num + w * v;  den = den + w
 *               out = num / den
 *     The kernel is a gather (a thread owns canvas pixels and loops over their tiles; no atomics, nothing accumulated
 *     across launches), so canvas_dev (N,H,W,C) is a function of the tiles alone, and every pixel is written exactly
 *     once.  gt_canvas_dev != NULL: the same pass writes the seven RangeInvariantPsnr sums of dsx_stitch_psnr per
 *     (frame, workgroup, channel) into partials_dev [N][dsx_tileplan_blend_blocks][C][8] (C <= 4), through the
 *     fixed-order block reduction: equal inputs give equal bits.
 *     Null pointers, C < 1, world < 1, a plan that does not cover its frames, a plan without a window, more than 65535
 *     frames, C * ph * pw beyond 32 bits and a rank_stride_elems below rank 0's whole tiles are DSX_ERR_INVALID before
 *     any HIP call.  No allocation, copy or synchronisation per call (the tables and the window go up at first use).
 *   dsx_tileplan_gather_canvas: the inverse cut -- the tiles first + k*stride, k < count, of the plan out of a
 *     multi-channel frame state canvas_dev (N,H,W,C) -> tiles_dev (count, C, ph, pw), bit for bit the slices.  Refusals
 *     as dsx_tileplan_randn's, under the name tileplan_gather_canvas.
 *   dsx_tileplan_blend_step: one reverse step of a whole frame state with the BLEND of the tiles as its x0 -- frame
 *     diffusion for samplers whose update is affine in the network output with coefficients shared by the batch (the
 *     InDI family).  x0_tiles_dev: the tiles in one of dsx_tileplan_blend's two layouts; state_dev (N,H,W,C) is
 *     updated IN PLACE and must not alias the tiles.  Per canvas pixel (n, y, x) and channel c, fp32, every operation
 *     rounded on its own (no fma):
 *         v    = what dsx_tileplan_blend would write there (ascending tile id, num / den correctly rounded, a pixel
 *                with one contributor is a copy)
 *         mean = c_x0 * v + c_xt * X
 *         out  = sigma == 0 ? mean : mean + z * sigma          (dsx_posterior_step's rules with predict_eps == 0)
 *         z    = field(seed, id_base + n, draw)[c, y, x]: component j % 4 of Philox block j / 4 of the stream
 *                (seed, ((id_base + n) << 24) | draw), j = (c*H + y)*W + x -- bitwise what dsx_randn_samples writes
 *                for that frame and dsx_tileplan_randn crops.  With sigma == 0 nothing is generated.
 *     A gather like the blend: the thread that owns a pixel reads its state once and writes it once; no atomics, no
 *     LDS.  Everything dsx_tileplan_blend refuses, a null state, id_base + (N - 1) >= DSX_STREAM_ID_LIMIT,
 *     draw >= DSX_STREAM_DRAW_LIMIT and a non-finite coefficient are DSX_ERR_INVALID before any HIP call. */
int dsx_tileplan_contributors(const dsx_tileplan* plan, int32_t* rows /*[H][2]*/, int32_t* cols /*[W][2]*/);
int dsx_tileplan_set_window(dsx_tileplan* plan, const float* wy_host /*ph*/, const float* wx_host /*pw*/);
int dsx_tileplan_blend_blocks(const dsx_tileplan* plan);
int dsx_tileplan_blend(dsx_tileplan* plan, const float* tiles_dev, int C, int world, int64_t rank_stride_elems,
                       float* canvas_dev, const float* gt_canvas_dev, double* partials_dev, void* stream);
int dsx_tileplan_gather_canvas(dsx_tileplan* plan, const float* canvas_dev, int C, int64_t first, int64_t stride,
                               int64_t count, float* tiles_dev, void* stream);
int dsx_tileplan_blend_step(dsx_tileplan* plan, const float* x0_tiles_dev, int C, int world, int64_t rank_stride_elems,
                            float* state_dev, float c_x0, float c_xt, float sigma, uint64_t seed, uint64_t id_base,
                            uint32_t draw, void* stream);
/* Tile disagreement: how far the tiles that predicted a canvas pixel differ -- what a blend hides and a crop-paste
 * switches between.  It needs no ground truth.  The plan must cover its frames with one frame per tile
 * (dsx_tileplan_blend's condition; no window is needed).  For canvas pixel (n, y, x) and channel c let v_1 .. v_k be its
 * contributors in ASCENDING TILE ID.  In double, every operation rounded on its own (no fma) -- the recurrence of
 * dsx_moments_update / dsx_moments_finish:
 *     mean = v_1; M2 = 0
 *     for r = 1 .. k-1:   d = v_{r+1} - mean;  mean = mean + d / (r + 1);  M2 = M2 + d * (v_{r+1} - mean)
 *     var = k > 1 ? M2 / (k - 1) : 0          s = (float)sqrt(var)
 * var is the unbiased variance among the tiles that predicted the pixel; 2 var is the mean squared difference over all
 * pairs of contributors, so sqrt(2 * mean(var)) is an RMS pairwise difference.
 *   Crop lines.  The plan's clipped paste regions (dsx_tileplan_regions) partition every frame.  A canvas column x >= 1 is
 *   a crop line if the tile column that owns x differs from the one that owns x - 1; rows alike.  With half-width `band`
 *   (1..65535) column x is NEAR A LINE if some crop line L has L - band <= x < L + band; rows alike.  A pixel is IN THE
 *   BAND if k >= 2 and its column or its row is near a line: where a crop-pasted frame switches from one tile to another.
 *   dsx_tileplan_crop_lines: host only; rows [H] and cols [W] = 1 where the row / column is near a line, else 0.
 *   dsx_tileplan_disagreement: tiles_dev in one of dsx_tileplan_blend's two layouts.  map_dev (N,H,W,C) receives s, or is
 *     NULL.  partials_dev [N][dsx_tileplan_blend_blocks][C][8] receives per (frame, workgroup, channel), through the
 *     fixed-order block reduction, over the workgroup's pixels:
 *         0  count of pixels with k >= 2 (exact)        1  sum of var over those pixels
 *         2  count of band pixels (exact)               3  sum of var over band pixels
 *         4 / 5  min / max of var over pixels with k >= 2; +inf / -inf if none        6, 7  0
 *     A gather like the blend: no atomics, nothing accumulated across launches, equal inputs give equal bits, and the
 *     result depends on the tiles alone, not on their layout.  The masks of a band go up at the first call that names
 *     it and stay with the plan: no allocation, copy or synchronisation per call after that.
 *     Everything dsx_tileplan_blend refuses except a missing window, null tiles or partials, C outside 1..4 and band
 *     outside 1..65535 are DSX_ERR_INVALID before any HIP call. */
int dsx_tileplan_crop_lines(const dsx_tileplan* plan, int band, uint8_t* rows /*[H]*/, uint8_t* cols /*[W]*/);
int dsx_tileplan_disagreement(dsx_tileplan* plan, const float* tiles_dev, int C, int world, int64_t rank_stride_elems,
                              int band, float* map_dev, double* partials_dev, void* stream);

/* ------------------------------------------------- frame files: uncompressed TIFF / BigTIFF stacks (host only)
 * Replaces imread(fpath, plugin='tifffile') of the Hagen loaders (data/split_dataset.py:76-91) for the files the
 * reference's configs name, and writes the stitched prediction.  Works without a GPU.
 * Read: classic TIFF (magic 42) and BigTIFF (43), both byte orders, an IFD chain of equally shaped pages, strips with
 * any RowsPerStrip, Compression = 1, BitsPerSample 8 / 16 / 32 unsigned and 32-bit float, SamplesPerPixel 1..4 chunky,
 * and ImageJ's contiguous stack (a single IFD whose ImageDescription starts with "ImageJ=" and carries "images=N",
 * page 0's strips contiguous and the file long enough for N planes from StripOffsets[0]: how stacks past 4 GiB are
 * stored).  Tiles, PlanarConfiguration = 2, any compression, pages of differing shape or type and other bit depths are
 * refused, the message naming the tag's value.  Every offset and count of the file is checked against its size before
 * use: a truncated or inconsistent file is DSX_ERR_INVALID with a message, never a short read.
 * dsx_tiff_info: shape = {pages, H, W, samples}, *dtype = DSX_PIX_*.  dsx_tiff_read: pages [first_page, first_page +
 * n_pages) into dst_host (capacity in bytes) in the host's byte order, page-major, rows top to bottom, samples
 * interleaved. */
enum { DSX_PIX_U8 = 0, DSX_PIX_U16 = 1, DSX_PIX_U32 = 2, DSX_PIX_F32 = 3 };
typedef struct dsx_tiff dsx_tiff;
int dsx_tiff_open(const char* path, dsx_tiff** out);
int dsx_tiff_info(const dsx_tiff* h, int64_t shape[4], int* dtype);
int dsx_tiff_read(dsx_tiff* h, int64_t first_page, int64_t n_pages, void* dst_host, size_t capacity);
void dsx_tiff_close(dsx_tiff* h);
/* data_host (pages, H, W) of DSX_PIX_U8 / U16 / F32, one sample per pixel -> little-endian uncompressed pages of one
 * strip each, the pixel data of all pages back to back (readable as an ImageJ contiguous stack too).  description (may
 * be NULL) becomes page 0's ImageDescription.  bigtiff: 0 classic (refused past 4 GiB), 1 BigTIFF, -1 BigTIFF only
 * when the file passes 4 GiB. */
int dsx_tiff_write(const char* path, const void* data_host, int64_t pages, int64_t H, int64_t W, int dtype,
                   const char* description, int bigtiff);

/* ------------------------------------------------- frame statistics on the device
 * dst = (float)min(src, upper_clip) for `count` uint8 / uint16 values (src_dtype = DSX_PIX_U8 / DSX_PIX_U16;
 * upper_clip < 0: no clip): the hard-coded data[data > 1993.0] = 1993.0 of _load_data_channelwise_fpath
 * (data/split_dataset.py:80-82) and the widening to the fp32 the tile kernels read, applied to the stack as uploaded in
 * its file width.  Asynchronous on `stream`. */
int dsx_frames_to_f32(const void* src_dev, int src_dtype, int64_t count, double upper_clip, float* dst_dev, void* stream);
/* Order statistics for np.quantile of compute_normalization_dict (data/split_dataset.py:58-64) without a sort: for each
 * 0-based rank the rank-th smallest key over `count` elements, key = (double)a[i] (b_dev NULL) or
 * (double)a[i]*w0 + (double)b[i]*w1 with both products and the sum rounded on their own (never an fma): numpy's
 * t1*w0 + t2*w1 on float64 arrays.  Most-significant-digit radix select over the order-preserving integer image of the
 * key: every pass reads the sources once and histograms one digit of the elements under the current prefix (LDS
 * counters per workgroup, one 64-bit global atomic per non-empty bin); no per-element temporary.  The counts are
 * integers: the result is exact and run-to-run identical.  Inputs must be finite (NaN: undefined).  1 <= count <= 2^40,
 * 1 <= n_ranks <= 4096, ranks in [0, count) (host array, any order, repeats allowed).  workspace_dev holds
 * dsx_order_stats_workspace_bytes(count, n_ranks) bytes.  out_host[n_ranks] is complete on return (the call
 * synchronises the stream once per pass). */
size_t dsx_order_stats_workspace_bytes(int64_t count, int n_ranks);
int dsx_order_stats(const float* a_dev, const float* b_dev, int64_t count, double w0, double w1, const int64_t* ranks,
                    int n_ranks, double* out_host, void* workspace_dev, void* stream);

/* ------------------------------------------------- refining the mixing time from the split itself
 * The centred second moments of `planes` plane triples (g, p1, p2), n fp32 pixels each, in one pass: all that
 * RangeInvariantPsnr(g, a p1 + b p2) (core/psnr.py:70-82) needs of the three planes, for ANY weights (a, b) -- the scan
 * of core/psnr_based_t_refinement.py:41-57 without re-reading a plane per grid point.  strides = {plane, pixel} element
 * strides of g, p1 and p2, so that a (b, 1, p, p) tile tensor, one channel of a (b, 2, p, p) tensor and one channel of a
 * channel-last (N, H, W, 2) canvas are read in place.  out_dev receives 12 doubles per plane:
 *   {n, min g, max g, mean g, mean p1, mean p2, Cgg, C11, C22, Cg1, Cg2, C12},   Cxy = sum (x - mean x)(y - mean y)
 * The curve, for the caller to evaluate in double (core.psnr.range_invariant_psnr_curve does):
 *   var  = Cgg / (n - 1)                                  (the ddof = 1 standardisation of RangeInvariantPsnr)
 *   gp   = a Cg1 + b Cg2,    pp = a^2 C11 + 2 a b C12 + b^2 C22
 *   mse  = ((n - 1) - gp^2 / (var pp)) / n
 *   PSNR = 10 log10((max g - min g)^2 / var / mse)        NaN where min g == max g or pp <= 0; an mse that rounding
 *                                                         takes below 0 (an exact fit) counts as 0: +inf
 * and its continuous maximiser over p = t p1 + (1 - t) p2:  u = S^-1 c,  S = [[C11, C12], [C12, C22]],  c = (Cg1, Cg2),
 * t* = u0 / (u0 + u1)  (NaN when S is singular or u0 + u1 == 0; not clamped to [0, 1]).
 * Centring: ONE pass on data shifted by the first element of each plane, x' = (double)x[i] - (double)x[0]; sums of x'
 * and of the six products accumulate in double (fma allowed), then mean x = x[0] + Sx / n, Cxy = Sxy - Sx Sy / n.  The
 * contract is an error bound (tests/comoments_ref.py derives it) plus repeatability, not numpy's bits.  A plane is cut
 * into dsx_comoments_blocks(n) workgroups, a function of n alone, each thread takes fixed pixels in a fixed order and
 * nothing is an atomic: a plane's 12 numbers have the same bits run to run, at any position in a call, in a call of any
 * number of planes and on either load path (16-byte loads when every pixel stride is 1, every base is 16-byte aligned,
 * every plane stride is a multiple of 4 and n % 4 == 0; 4-byte loads otherwise).  Planes are assumed finite.
 * partial_dev holds planes * dsx_comoments_blocks(n) * 12 doubles.  Two launches on `stream`, no synchronisation.
 * DSX_ERR_INVALID with a message, before any device work: a NULL pointer, n < 1, planes outside 0..65535 (0: DSX_OK,
 * nothing is done and no device is needed), a stride < 1, planes > 1 with a plane stride < (n - 1) * pixel stride + 1
 * (the planes of that operand would overlap). */
int dsx_comoments_blocks(int64_t n);
int dsx_comoments(const float* g_dev, const float* p1_dev, const float* p2_dev, int64_t planes, int64_t n,
                  const int64_t strides[6], double* partial_dev, double* out_dev, void* stream);

/* ------------------------------------------------- calibrating the posterior spread: RMV-RMSE bins, coverage
 * Does a predicted per-pixel standard deviation track the real error?  The pixels of every channel are binned by their
 * predicted std, and per bin the sum of the predicted variances stands beside the sum of the squared errors; the
 * curve rmv_b = sqrt(Sv_b / count_b) against rmse_b = sqrt(Se_b / count_b), its fit and the interval coverage are the
 * caller's (core/calibration.py).  mean, std and target are channel-last canvases as predict_stack returns them:
 * n pixels of C interleaved fp32 channels ((N, H, W, C), n = N H W), read in place, once.  Per channel c and pixel i,
 * everything in double:
 *   s   = (double)std[i][c]
 *   e   = (double)target[i][c] - (double)mean[i][c]                 one rounding
 *   bin = #{ j : edges[c][j] <= s }                                 np.searchsorted(edges[c], s, side='right'), 0..nbins-1
 *   count[c][bin] += 1;   Sv[c][bin] += s * s;   Se[c][bin] += e * e
 *   cover[c][k]  += (s >= 0 && fabs(e) <= z[k] * s)   for k < nz    the product rounded once
 * edges_host = [C][nbins - 1], ascending per channel (ties allowed); z_host = [nz].  Both travel in the kernel-argument
 * struct, hence nbins <= 64 and nz <= 8.  out_dev receives C rows of 3 * nbins + nz doubles:
 *   {count, Sv, Se} of bin 0, .. of bin nbins - 1, then cover[0 .. nz - 1]
 * The contract: counts and coverage are exact integers (n <= 2^40), equal to a float64 numpy restatement; Sv and Se
 * lie within (k + 4) 2^-53 of the exactly rounded sum of the exactly formed terms, relative to it, k = the bin's count
 * (tests/calibration_ref.py derives it); a call's bits are the same run to run and on either load path (16-byte loads
 * when the three bases are 16-byte aligned and n C % 4 == 0; 4-byte loads otherwise).  The canvases are cut into
 * dsx_calibration_blocks(n) workgroups, a function of n alone, each thread takes fixed values in a fixed order, and
 * there is no floating-point atomic: a bin's terms meet in the wave's row of LDS, in ascending lane order or, where more
 * than 8 of a wave's 64 values share a bin, folded by one shuffle butterfly (csrc/dsx_calib.hip: the values alone
 * decide), the four waves pairwise, the workgroups' rows in ascending order.  Inputs are assumed finite.
 * A negative std is binned by its value and never counts as covered (not even z = 0 with e = 0).
 * partial_dev holds dsx_calibration_blocks(n) * C * (3 * nbins + nz) doubles.  Two launches on `stream`; the call does
 * not synchronise, allocate or copy.
 * DSX_ERR_INVALID with a message, before any device work: a NULL pointer (edges_host may be NULL when nbins == 1,
 * z_host when nz == 0), n outside 1..2^40, C outside 1..4, nbins outside 1..64, nz outside 0..8, an edge that is not
 * finite, edges that descend, a z that is not finite or negative. */
int dsx_calibration_blocks(int64_t n);
int dsx_calibration(const float* mean_dev, const float* std_dev, const float* target_dev, int64_t n, int C,
                    const double* edges_host, int nbins, const double* z_host, int nz, double* partial_dev, double* out_dev,
                    void* stream);

/* ------------------------------------------------- quantiles and ranks across a stack of posterior samples
 * The per-element order statistics of n samples, for maps of the median and of credible bands, and the rank of a
 * target among the samples, for the rank histogram (core/calibration.py) that checks such a band without assuming a
 * distribution.  x_dev holds n samples of `count` fp32 values: sample r, element i at x_dev[r * sample_stride + i],
 * sample_stride >= count.  out_dev is [nq][count]; target_dev and rank_dev are [count], both NULL or both given;
 * out_dev (and q_host) may be NULL with nq == 0 when only ranks are wanted.  Per element i:
 *   v[0 .. n-1] = the element's n samples in ascending order of the order-preserving integer image of the fp32 value:
 *                 -0 comes before +0, equal values are indistinguishable
 * on the host, in double, for every k < nq (the four travel in the kernel-argument struct, hence nq <= 8):
 *   pos = (n - 1) q[k];   lo = floor(pos);   hi = min(lo + 1, n - 1);   t = pos - lo
 * on the device, in double, every operation rounded on its own (no fma):
 *   a = v[lo];   b = v[hi];   d = b - a
 *   r = t < 0.5 ? a + d t : b - d (1 - t)
 *   out[k][i] = (float)r
 * which is np.quantile(x.astype(np.float64), q, axis=0).astype(np.float32) bit for bit (tests/quantile_ref.py), the
 * expression dsx_order_stats' callers use on the host.
 *   rank[i] = (float)#{ r : x_r[i] < target[i] }      strict, on the fp32 values: an exact integer in 0..n
 * Inputs are assumed finite.  The samples are sorted in registers by a fully unrolled compare-exchange network over
 * n padded to 2, 4, .. 64 wires (csrc/dsx_quantiles.hip), hence n <= 64.  A call's bits do not depend on the load path
 * (loads of 16 bytes, 8 at n > 32, when every base, sample_stride and count are multiples of that; 4-byte loads
 * otherwise), on alignment or on sample_stride.  One launch on `stream`; the call does not synchronise, allocate or copy
 * beyond the argument struct.
 * DSX_ERR_INVALID with a message, before any device work: a NULL x_dev, n outside 1..64, nq outside 0..8, nq == 0
 * without a rank output, nq > 0 without q_host and out_dev, count < 1, sample_stride < count, a q that is not finite
 * or lies outside [0, 1], only one of target_dev / rank_dev, out_dev or rank_dev overlapping the samples' range. */
int dsx_sample_quantiles(const float* x_dev, int64_t sample_stride, int n, int64_t count, const double* q_host, int nq,
                         float* out_dev, const float* target_dev, float* rank_dev, void* stream);

/* ------------------------------------------------- data consistency of a split: residual, report row, projection
 * The network's input is, by construction, x = sum_c w_c p_c in raw counts, so a split of an acquisition must add back
 * up to it.  One pass over `frames` frames of `plane` = H W pixels forms the residual r = x - sum_c w_c p_c of a
 * prediction, a report row per frame, and the prediction conditioned on the observation: an independent Gaussian
 * posterior N(p_c, v_c) conditioned on sum_c w_c t_c = x with noise variance noise_var.
 *   input_dev     (frames, plane) of `pix` = DSX_PIX_U8 / DSX_PIX_U16 / DSX_PIX_F32, the acquisition in its file width
 *   mean_dev      (frames, plane, C) fp32, channel-last, normalised, as predict_stack returns it; C in 1..4
 *   std_dev       the same shape, or NULL
 *   scale_host[C] = a_c (std_target), shift_host[C] = b_c (mean_target), weight_host[C] = w_c
 *   clip < 0: none;  noise_var = rho^2 >= 0
 * Outputs, each may be NULL (not all): map_dev (frames, plane) fp32; out_mean_dev, out_std_dev (frames, plane, C) fp32,
 * normalised; out_dev [frames][10] doubles, which needs partial_dev of frames * dsx_consistency_blocks(plane) * 10
 * doubles.  Per pixel, in double, every operation rounded on its own (no fma), channels in ascending order:
 *   x   = (double)input
 *   sat = clip >= 0 && x >= clip
 *   p_c = (double)mean[c] * a_c + b_c
 *   m   = sum_c w_c * p_c                              ((0 + w_0 p_0) + w_1 p_1) + ..
 *   r   = x - m
 *   map = (float)r                                     written for every pixel, saturated ones too
 *   v_c = std ? ((double)std[c] * a_c)^2 : 1.0
 *   den = sum_c (w_c * w_c) * v_c + noise_var          the sum over c first, then + noise_var
 *   if (!sat && den > 0):
 *     p'_c        = p_c + ((v_c * w_c) * r) / den
 *     out_mean[c] = (float)((p'_c - b_c) / a_c)
 *     v'_c        = v_c - ((v_c * w_c) * (v_c * w_c)) / den
 *     out_std[c]  = (float)(sqrt(max(v'_c, 0)) / a_c)
 *   else:
 *     out_mean[c] = mean[c]                            the input's fp32 bits, copied
 *     out_std[c]  = std ? std[c] : 0                   copied likewise
 * A saturated pixel only says sum_c w_c p_c >= clip, so it is left alone and counted.  With std == NULL and
 * noise_var == 0 the update is the orthogonal projection onto the constraint.  The row of a frame, over its pixels:
 *   0  count of unsaturated pixels k          1  count of saturated pixels              (exact)
 *   2  sum r      3  sum r * r      4  sum x      5  sum x * x                          over the unsaturated pixels
 *   6  count of unsaturated pixels with den > 0      7  sum (r * r) / den over those
 *   8  min r      9  max r                    over the unsaturated pixels (+inf, -inf if none)
 * The contract: map, out_mean and out_std equal a float64 numpy restatement bit for bit (tests/consistency_ref.py);
 * counts, min and max are exact; the sums of non-negative terms lie within (k + 4) 2^-53 of the exactly rounded sum of
 * the same terms, relative to it, and sum r within that factor times sum |r|.  A frame is cut into
 * dsx_consistency_blocks(plane) workgroups, a function of plane alone, each thread takes fixed pixels in a fixed order,
 * the rows meet by dsx_reduce.h (kDown, Pairwise) and the workgroup rows in ascending order; there is no atomic.  So a
 * call's bits do not depend on the load path (four pixels per thread with 16-byte accesses of the fp32 operands and one
 * 4-, 8- or 16-byte load of the input when every base is that aligned and plane % 4 == 0; single accesses otherwise), on
 * alignment, on a frame's position in the call or on the number of frames.  Inputs are assumed finite.
 * Aliasing: the outputs may alias nothing but themselves, with one exception, in place: out_mean_dev == mean_dev and
 * out_std_dev == std_dev exactly (a thread reads its pixels before it writes them).  Any other overlap of an output
 * with an input or with another output is refused.
 * Two launches on `stream` (one when out_dev is NULL); the call does not synchronise, allocate or copy.
 * DSX_ERR_INVALID with a message, before any device work: a NULL input_dev, mean_dev or host array, out_dev without
 * partial_dev, frames outside 1..65535, plane < 1, C outside 1..4, an unknown pix (DSX_PIX_U32 included), an a_c that
 * is not > 0, a scalar that is not finite, noise_var < 0, every w_c == 0, out_std_dev without std_dev, no output at all,
 * an overlap as above. */
int dsx_consistency_blocks(int64_t plane);
int dsx_consistency(const void* input_dev, int pix, const float* mean_dev, const float* std_dev, int64_t frames,
                    int64_t plane, int C, const double* scale_host, const double* shift_host, const double* weight_host,
                    double clip, double noise_var, float* map_dev, float* out_mean_dev, float* out_std_dev,
                    double* out_dev, double* partial_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSX_H */
