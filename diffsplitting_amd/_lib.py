"""ctypes binding of libdsx.so (C ABI: include/dsx.h).

The HIP library is the product path; there is no CPU fallback.  Importing this
module without a built ``libdsx.so`` raises, and every compute entry point
raises ``DsxError`` when no MI355X is visible.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSX_LIB_PATH: diagnostic builds of the SAME library (tools/build_variant.sh: ablation / stamp builds) for
# timing experiments; never a different implementation
LIB_PATH = os.environ.get("DSX_LIB_PATH") or os.path.join(_HERE, "libdsx.so")


class DsxError(RuntimeError):
    pass


class UnetCfg(C.Structure):
    _fields_ = [("flavour", C.c_int32), ("in_channel", C.c_int32), ("out_channel", C.c_int32),
                ("inner_channel", C.c_int32), ("norm_groups", C.c_int32), ("n_mults", C.c_int32),
                ("channel_mults", C.c_int32 * 8), ("n_attn_res", C.c_int32), ("attn_res", C.c_int32 * 8),
                ("res_blocks", C.c_int32), ("image_size", C.c_int32), ("with_time_emb", C.c_int32)]


class StepTable(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("predict_eps", C.c_int32), ("clip", C.c_int32),
                ("tcond", C.POINTER(C.c_float)), ("a", C.POINTER(C.c_float)), ("b", C.POINTER(C.c_float)),
                ("c1", C.POINTER(C.c_float)), ("c2", C.POINTER(C.c_float)), ("sigma", C.POINTER(C.c_float)),
                ("per_sample", C.c_int32)]


class LayerInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "op_begin", "op_end", "op_main", "ks", "stride", "up", "swish", "B", "Hs", "Ws", "Ho", "Wo",
        "C0", "C1", "src_dtype", "gn_gamma_param", "gn_beta_param", "gn_in_kernel", "w_param", "b_param",
        "bias_in_film", "film_off", "film_bs", "resid_ld", "out_ld", "Cout", "out_dtype", "ld", "reserved")] + \
        [(n, C.c_uint64) for n in ("src0", "src1", "gn_scale", "gn_shift", "film", "resid", "out")]


FLAVOUR_SR3, FLAVOUR_DDPM = 0, 1
LAYER_CONV, LAYER_ATTN, LAYER_FILM, LAYER_INPUT = 0, 1, 2, 3
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
TILING_TRIM, TILING_PAD, TILING_SHIFT = 0, 1, 2
STREAM_ID_LIMIT, STREAM_DRAW_LIMIT = 1 << 40, 1 << 24      # per-sample noise streams: id < 2^40, draw < 2^24
RESIZE_BILINEAR, RESIZE_BICUBIC = 2, 3
PIX_U8, PIX_U16, PIX_U32, PIX_F32 = 0, 1, 2, 3

_vp, _i, _i64, _u64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float
_pi64, _pi32, _pf = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
_pu64 = C.POINTER(C.c_uint64)

# name -> (restype, argtypes); exactly the declarations of include/dsx.h
SIGNATURES = {
    "dsx_last_error": (C.c_char_p, []),
    "dsx_abi_version": (_i, []),
    "dsx_device_count": (_i, []),
    "dsx_model_create": (_i, [C.POINTER(UnetCfg), C.POINTER(_vp)]),
    "dsx_model_destroy": (None, [_vp]),
    "dsx_model_num_params": (_i, [_vp]),
    "dsx_model_param_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_i), _pi64]),
    "dsx_model_set_param": (_i, [_vp, _i, _vp, _i64]),
    "dsx_model_set_posenc_freq": (_i, [_vp, _vp, _i]),
    "dsx_model_finalize": (_i, [_vp, _i]),
    "dsx_model_packed_bytes": (_i, [_vp, _i, C.POINTER(C.c_size_t)]),
    "dsx_model_export_packed": (_i, [_vp, _vp, C.c_size_t]),
    "dsx_model_finalize_packed": (_i, [_vp, _i, _vp, C.c_size_t]),
    "dsx_model_flops": (C.c_double, [_vp, _i, _i]),
    "dsx_exec_create": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_vp)]),
    "dsx_exec_destroy": (None, [_vp]),
    "dsx_exec_workspace_bytes": (C.c_size_t, [_vp]),
    "dsx_exec_handoff_timeouts": (_i, [_vp, C.POINTER(C.c_uint)]),
    "dsx_plan_dry_run": (_i, [C.POINTER(UnetCfg), _i, _i, _i, _i, _i, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                              C.POINTER(_i)]),
    "dsx_exec_num_launches": (_i, [_vp]),
    "dsx_exec_num_ops": (_i, [_vp]),
    "dsx_exec_op_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsx_exec_profile": (_i, [_vp, _i, _vp, _vp]),
    "dsx_exec_time_kind": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "dsx_exec_read_stamps": (_i, [_vp, _vp]),
    "dsx_exec_num_layers": (_i, [_vp]),
    "dsx_exec_layer_info": (_i, [_vp, _i, C.POINTER(LayerInfo)]),
    "dsx_exec_copy_workspace": (_i, [_vp, _u64, C.c_size_t, _vp, _vp]),
    "dsx_unet_forward": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "dsx_time_predictor_set_mask": (_i, [_vp, _vp, _vp]),
    "dsx_time_predictor_forward": (_i, [_vp, _vp, _vp, _vp]),
    "dsx_sample_loop": (_i, [_vp, C.POINTER(StepTable), _vp, _vp, _vp, _u64, _pi32, _i, _vp, _i, _vp]),
    "dsx_sr3_step": (_i, [_vp, _f, _f, _f, _f, _f, _f, _i, _vp, _vp, _vp, _u64, _vp]),
    "dsx_indi_step": (_i, [_vp, _f, _f, _f, _f, _vp, _vp, _u64, _vp]),
    "dsx_randn": (_i, [_vp, _i64, _u64, _u64, _vp]),
    "dsx_q_sample": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _i, _i, _vp]),
    "dsx_loss_blocks": (_i, [_i, _i, _i]),
    "dsx_loss": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "dsx_attention": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "dsx_posterior_step": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _u64, _u64, _i, _vp, _vp,
                                _vp, _vp]),
    "dsx_interp_start": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _u64, _u64, _vp, _vp]),
    "dsx_randn_samples": (_i, [_vp, _i, _i64, _u64, _pu64, C.c_uint32, _vp]),
    "dsx_sample_loop_streams": (_i, [_vp, C.POINTER(StepTable), _vp, _vp, _vp, _u64, _pi32, _i, _vp, _i, _vp, _pu64, _i]),
    "dsx_posterior_step_streams": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _u64, _u64, _i, _vp,
                                        _vp, _vp, _vp, _pu64, _i]),
    "dsx_val_report": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_double, C.c_double, C.POINTER(C.c_double),
                            C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsx_tile_plan": (_i64, [_pi64, _pi64, _pi64, _i, _pi64, _pi64, _i64]),
    "dsx_tile_regions": (_i, [_pi64, _pi64, _pi64, _i, _pi32, _i64]),
    "dsx_tiles_gather": (_i, [_vp, _pi64, _pi64, _pi64, _pi64, _i64, _vp, _vp]),
    "dsx_tiles_gather_norm": (_i, [_vp, _vp, _pi64, _pi64, _pi64, _pi64, _i64, _f, _f, C.POINTER(C.c_double), _i, _vp, _vp, _vp]),
    "dsx_tiles_gather_norm_planes": (_i, [_vp, _vp, _pi64, _pi64, _pi64, _pi64, _i64, _f, _f, C.c_double, C.c_double,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), _vp, _vp, _vp]),
    "dsx_tiles_gather_mix": (_i, [_vp, _vp, _pi64, _pi64, _pi64, _pi64, _i64, C.POINTER(C.c_double), C.c_double,
                                  C.POINTER(C.c_double), _vp, _vp, _vp, _vp]),
    "dsx_tiles_gather_mix_items": (_i, [_vp, _vp, _pi64, _pi64, _pi64, _i64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), _vp, _vp, _vp, _vp]),
    "dsx_mix_range_blocks": (_i, [_i64, _i]),
    "dsx_mix_range": (_i, [_vp, _vp, _i64, C.POINTER(C.c_double), _i, _vp, C.POINTER(C.c_double), _vp]),
    "dsx_stitch": (_i, [_vp, _i64, _i, _i, _i, _pi32, _vp, _pi64, _vp]),
    "dsx_stitch_psnr_blocks": (_i, [_i, _i]),
    "dsx_stitch_psnr": (_i, [_vp, _i64, _i, _i, _i, _pi32, _vp, _pi64, _vp, _vp, _vp]),
    "dsx_image_metrics_blocks": (_i, [_i, _i]),
    "dsx_image_metrics": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp,
                               C.POINTER(C.c_double), C.POINTER(C.c_double), _vp]),
    "dsx_lpips_create": (_i, [C.POINTER(_vp), _pi64, C.POINTER(_vp), _pi64, C.POINTER(_vp)]),
    "dsx_lpips_destroy": (None, [_vp]),
    "dsx_lpips_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "dsx_lpips_frames": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "dsx_resize_coeffs": (_i, [_i, _i, _i, _pi32, _pi32, _pi32, _i]),
    "dsx_resize_plan_create": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "dsx_resize_plan_destroy": (None, [_vp]),
    "dsx_resize_workspace_bytes": (C.c_size_t, [_vp, _i]),
    "dsx_resize_u8": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "dsx_u8_to_tensor": (_i, [_vp, _i, _i, _i, _i, _f, _f, _vp, _vp]),
    "dsx_tileplan_create": (_i, [_pi64, _pi64, _pi64, _i, C.POINTER(_vp)]),
    "dsx_tileplan_destroy": (None, [_vp]),
    "dsx_tileplan_total": (_i64, [_vp]),
    "dsx_tileplan_regions": (_i, [_vp, _pi32, _i64]),
    "dsx_tileplan_gather": (_i, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "dsx_tileplan_gather_norm": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _f, _f, C.POINTER(C.c_double), _i, _vp, _vp, _vp]),
    "dsx_tileplan_gather_mix": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, C.POINTER(C.c_double), C.c_double,
                                     C.POINTER(C.c_double), _vp, _vp, _vp, _vp]),
    "dsx_tileplan_gather_input": (_i, [_vp, _vp, _i, _i64, _i64, _i64, C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "dsx_moments_update": (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    "dsx_moments_finish": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "dsx_tileplan_stitch": (_i, [_vp, _vp, _i, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "dsx_tileplan_pack_layout": (_i, [_vp, _i, _pi64, _pi64]),
    "dsx_tileplan_pack": (_i, [_vp, _vp, _i, _i, _i64, _i64, _vp, _vp]),
    "dsx_tileplan_paste_packed": (_i, [_vp, _vp, _i, _i, _i64, _vp, _vp, _vp, _vp]),
    "dsx_tiff_open": (_i, [C.c_char_p, C.POINTER(_vp)]),
    "dsx_tiff_info": (_i, [_vp, _pi64, C.POINTER(_i)]),
    "dsx_tiff_read": (_i, [_vp, _i64, _i64, _vp, C.c_size_t]),
    "dsx_tiff_close": (None, [_vp]),
    "dsx_tiff_write": (_i, [C.c_char_p, _vp, _i64, _i64, _i64, _i, C.c_char_p, _i]),
    "dsx_frames_to_f32": (_i, [_vp, _i, _i64, C.c_double, _vp, _vp]),
    "dsx_order_stats_workspace_bytes": (C.c_size_t, [_i64, _i]),
    "dsx_order_stats": (_i, [_vp, _vp, _i64, C.c_double, C.c_double, _pi64, _i, C.POINTER(C.c_double), _vp, _vp]),
}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). There is no CPU fallback for the sampling path.")

lib = C.CDLL(LIB_PATH)
for _name, (_res, _args) in SIGNATURES.items():
    try:
        _fn = getattr(lib, _name)
    except AttributeError:
        if "DSX_LIB_PATH" not in os.environ:
            raise                      # the product library must export everything include/dsx.h declares
        # a diagnostic variant (tools/build_variant.sh) built before an entry point was added: usable for timing
        # experiments, the missing call fails loudly if it is ever made
        def _missing(*_a, _n=_name, **_k):
            raise DsxError(f"{LIB_PATH} (DSX_LIB_PATH variant) does not export {_n}: rebuild the variant")
        setattr(lib, _name, _missing)
        continue
    _fn.restype = _res
    _fn.argtypes = _args


def check(rc):
    """Raise DsxError with the library's message on a negative status."""
    if rc is not None and rc < 0:
        raise DsxError(f"libdsx status {rc}: {lib.dsx_last_error().decode(errors='replace')}")
    return rc


def require_gpu():
    if lib.dsx_device_count() < 1:
        raise DsxError("no HIP device visible: the sampling path runs on MI355X only (no CPU fallback)")
