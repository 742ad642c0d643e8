"""ctypes binding of libdsx.so (C ABI: include/dsx.h).

The HIP library is the product path; there is no CPU fallback.  Importing this
module without a built ``libdsx.so`` raises, and every compute entry point
raises ``DsxError`` when no MI355X is visible.
"""
import collections
import ctypes as C
import os
import types

import numpy as np
import torch

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


class SolverTable(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("clip", C.c_int32)] + \
        [(n, C.POINTER(C.c_float)) for n in ("tcond", "a", "b", "cx", "c0", "cp", "sigma")]


class LayerInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "op_begin", "op_end", "op_main", "ks", "stride", "up", "swish", "B", "Hs", "Ws", "Ho", "Wo",
        "C0", "C1", "src_dtype", "gn_gamma_param", "gn_beta_param", "gn_in_kernel", "w_param", "b_param",
        "bias_in_film", "film_off", "film_bs", "resid_ld", "out_ld", "Cout", "out_dtype", "ld", "reserved")] + \
        [(n, C.c_uint64) for n in ("src0", "src1", "gn_scale", "gn_shift", "film", "resid", "out")]


class LpipsLayerTable(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("nimg", C.c_int32), ("H", C.c_int32 * 8), ("W", C.c_int32 * 8),
                ("C", C.c_int32 * 8), ("nblk", C.c_int32 * 5), ("hw", C.c_int32 * 5), ("stage", C.c_uint64 * 8),
                ("part", C.c_uint64 * 5)]


FLAVOUR_SR3, FLAVOUR_DDPM = 0, 1
LAYER_CONV, LAYER_ATTN, LAYER_FILM, LAYER_INPUT = 0, 1, 2, 3
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
TILING_TRIM, TILING_PAD, TILING_SHIFT = 0, 1, 2
STREAM_ID_LIMIT, STREAM_DRAW_LIMIT = 1 << 40, 1 << 24      # per-sample noise streams: id < 2^40, draw < 2^24
RESIZE_BILINEAR, RESIZE_BICUBIC = 2, 3
PIX_U8, PIX_U16, PIX_U32, PIX_F32 = 0, 1, 2, 3


class _Kind(collections.namedtuple("_Kind", "name elem", defaults=(None,))):
    """What a ``void*`` of include/dsx.h stands for; passed to C as a plain address.  Equal when they mean the same."""
    ctype = C.c_void_p


# Dev(elem): device memory of the header's element type.  None -> NULL; a tensor must be CUDA, contiguous and of one of
# these dtypes (an integer type: either signedness of its width, torch versions differ in the unsigned ones; void:
# anything) and yields its address; an int or c_void_p is an address the caller already holds: passed unchanged.
Dev = lambda elem: _Kind("Dev", elem)
_ints = lambda bits: tuple(getattr(torch, f"{u}int{bits}") for u in ("", "u") if hasattr(torch, f"{u}int{bits}"))
DEV_DTYPES = {"float": (torch.float32,), "double": (torch.float64,), "uint8_t": _ints(8), "uint16_t": _ints(16),
              "uint64_t": _ints(64), "void": None}
# Host: host memory passed as bytes (None, C-contiguous numpy arrays, contiguous CPU tensors, ctypes objects, int).
# Handle: an opaque library object (c_void_p, int, None).  Stream: a HIP stream (a torch.cuda.Stream, an address, or
# None: the current stream of the call's device; NULL, the default stream, when the call has no tensor).
_H, _hn, _st = Host, Handle, Stream = _Kind("Host"), _Kind("Handle"), _Kind("Stream")

_vp, _i, _i64, _u64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float
_pi64, _pi32, _pu64 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
_Df, _Dd, _Dv, _D8, _D16, _D64 = (Dev(e) for e in ("float", "double", "void", "uint8_t", "uint16_t", "uint64_t"))

# name -> (restype, parameters): the declarations of include/dsx.h, with a kind where the header has a `T*` for memory, a
# handle or the stream; typed ctypes pointers are host arrays.  tests/test_binding_cpu.py holds every entry against its
# prototype: parameter count, pointer or scalar (width, signedness), the kind its name asks for, a Dev's element type.
SIGNATURES = {
    "dsx_last_error": (C.c_char_p, []),
    "dsx_abi_version": (_i, []),
    "dsx_device_count": (_i, []),
    "dsx_model_create": (_i, [C.POINTER(UnetCfg), C.POINTER(_vp)]),
    "dsx_model_destroy": (None, [_hn]),
    "dsx_model_num_params": (_i, [_hn]),
    "dsx_model_param_info": (_i, [_hn, _i, C.c_char_p, _i, C.POINTER(_i), _pi64]),
    "dsx_model_set_param": (_i, [_hn, _i, _H, _i64]),
    "dsx_model_set_posenc_freq": (_i, [_hn, _H, _i]),
    "dsx_model_finalize": (_i, [_hn, _i]),
    "dsx_model_packed_bytes": (_i, [_hn, _i, C.POINTER(C.c_size_t)]),
    "dsx_model_export_packed": (_i, [_hn, _H, C.c_size_t]),
    "dsx_model_finalize_packed": (_i, [_hn, _i, _H, C.c_size_t]),
    "dsx_model_flops": (C.c_double, [_hn, _i, _i]),
    "dsx_exec_create": (_i, [_hn, _i, _i, _i, _i, C.POINTER(_vp)]),
    "dsx_exec_destroy": (None, [_hn]),
    "dsx_exec_workspace_bytes": (C.c_size_t, [_hn]),
    "dsx_exec_handoff_timeouts": (_i, [_hn, C.POINTER(C.c_uint)]),
    "dsx_plan_dry_run": (_i, [C.POINTER(UnetCfg), _i, _i, _i, _i, _i, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                              C.POINTER(_i)]),
    "dsx_exec_num_launches": (_i, [_hn]),
    "dsx_exec_num_ops": (_i, [_hn]),
    "dsx_exec_op_info": (_i, [_hn, _i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsx_exec_profile": (_i, [_hn, _i, _H, _st]),
    "dsx_exec_time_kind": (_i, [_hn, _i, _i, _H, _H, _st]),
    "dsx_exec_read_stamps": (_i, [_hn, _H]),
    "dsx_exec_num_layers": (_i, [_hn]),
    "dsx_exec_layer_info": (_i, [_hn, _i, C.POINTER(LayerInfo)]),
    "dsx_exec_copy_workspace": (_i, [_hn, _u64, C.c_size_t, _Dv, _st]),
    "dsx_unet_forward": (_i, [_hn, _Df, _Df, _i, _Df, _st]),
    "dsx_time_predictor_set_mask": (_i, [_hn, _H, _H]),
    "dsx_time_predictor_forward": (_i, [_hn, _Df, _Df, _st]),
    "dsx_sample_loop": (_i, [_hn, C.POINTER(StepTable), _Df, _Df, _Df, _u64, _pi32, _i, _Df, _i, _st]),
    "dsx_sr3_step": (_i, [_hn, _f, _f, _f, _f, _f, _f, _i, _Df, _Df, _Df, _u64, _st]),
    "dsx_indi_step": (_i, [_hn, _f, _f, _f, _f, _Df, _Df, _u64, _st]),
    "dsx_randn": (_i, [_Df, _i64, _u64, _u64, _st]),
    "dsx_q_sample": (_i, [_Df, _Df, _i, _i, _i, _i, _i, _Df, _Df, _Df, _Df, _u64, _u64, _Df, _Df, _i, _i, _st]),
    "dsx_loss_blocks": (_i, [_i, _i, _i]),
    "dsx_loss": (_i, [_Df, _Df, _i, _i, _i, _i, _i, _Dd, _Dd, _st]),
    "dsx_attention": (_i, [_Dv, _i, _i, _i, _i, _Dv, _i, _i, _i, _i, _i, _i, _st]),
    "dsx_posterior_step": (_i, [_Df, _Df, _i, _i, _i, _i, _Df, _Df, _Df, _Df, _Df, _i, _i, _Df, _u64, _u64, _i, _Df, _Df, _Df,
                                _st]),
    "dsx_interp_start": (_i, [_Df, _Df, _i, _i, _i, _i, _Df, _Df, _f, _f, _Df, _Df, _u64, _u64, _Df, _st]),
    "dsx_randn_samples": (_i, [_Df, _i, _i64, _u64, _pu64, C.c_uint32, _st]),
    "dsx_sample_loop_streams": (_i, [_hn, C.POINTER(StepTable), _Df, _Df, _Df, _u64, _pi32, _i, _Df, _i, _st, _pu64, _i]),
    "dsx_posterior_step_streams": (_i, [_Df, _Df, _i, _i, _i, _i, _Df, _Df, _Df, _Df, _Df, _i, _i, _Df, _u64, _u64, _i, _Df,
                                        _Df, _Df, _st, _pu64, _i]),
    "dsx_solver_loop": (_i, [_hn, C.POINTER(SolverTable), _Df, _Df, _Df, _u64, _pi32, _i, _Df, _i, _st, _pu64, _i]),
    "dsx_solver_step": (_i, [_Df, _Df, _Df, _i, _i, _i, _i, _Df, _Df, _Df, _Df, _Df, _Df, _i, _Df, _u64, _u64, _Df, _Df, _st,
                             _pu64, _i, C.c_uint32]),
    "dsx_val_report": (_i, [_Df, _Df, _Df, _i, _i, _i, _i, _i, C.c_double, C.c_double, C.POINTER(C.c_double),
                            C.POINTER(C.c_double), _D16, _D16, _D16, _D16, _D16, _D16, _D64, _D64, _st]),
    "dsx_tile_plan": (_i64, [_pi64, _pi64, _pi64, _i, _pi64, _pi64, _i64]),
    "dsx_tile_regions": (_i, [_pi64, _pi64, _pi64, _i, _pi32, _i64]),
    "dsx_tiles_gather": (_i, [_Df, _pi64, _pi64, _pi64, _pi64, _i64, _Df, _st]),
    "dsx_tiles_gather_norm": (_i, [_Df, _Df, _pi64, _pi64, _pi64, _pi64, _i64, _f, _f, C.POINTER(C.c_double), _i, _Df, _Df,
                                   _st]),
    "dsx_tiles_gather_norm_planes": (_i, [_Df, _Df, _pi64, _pi64, _pi64, _pi64, _i64, _f, _f, C.c_double, C.c_double,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), _Df, _Df, _st]),
    "dsx_tiles_gather_mix": (_i, [_Df, _Df, _pi64, _pi64, _pi64, _pi64, _i64, C.POINTER(C.c_double), C.c_double,
                                  C.POINTER(C.c_double), _Df, _Df, _Df, _st]),
    "dsx_tiles_gather_mix_items": (_i, [_Df, _Df, _pi64, _pi64, _pi64, _i64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), _Df, _Df, _Df, _st]),
    "dsx_mix_range_blocks": (_i, [_i64, _i]),
    "dsx_mix_range": (_i, [_Df, _Df, _i64, C.POINTER(C.c_double), _i, _Dd, C.POINTER(C.c_double), _st]),
    "dsx_stitch": (_i, [_Df, _i64, _i, _i, _i, _pi32, _Df, _pi64, _st]),
    "dsx_stitch_psnr_blocks": (_i, [_i, _i]),
    "dsx_stitch_psnr": (_i, [_Df, _i64, _i, _i, _i, _pi32, _Df, _pi64, _Df, _Dd, _st]),
    "dsx_image_metrics_blocks": (_i, [_i, _i]),
    "dsx_image_metrics": (_i, [_Df, _Df, _i, _i, _i, _i, _i, C.c_double, C.c_double, C.c_double, _Dd, C.POINTER(C.c_double),
                               C.POINTER(C.c_double), _st]),
    "dsx_msssim_workspace": (_i64, [_i, _i, _i]),
    "dsx_msssim": (_i, [_Df, _Df, _i, _i, _i, _i, _i, C.c_double, _Dv, C.c_size_t, _H, _st]),
    "dsx_lpips_create": (_i, [C.POINTER(_vp), _pi64, C.POINTER(_vp), _pi64, C.POINTER(_vp)]),
    "dsx_lpips_destroy": (None, [_hn]),
    "dsx_lpips_forward": (_i, [_hn, _Df, _Df, _i, _i, _i, _Df, _Df, _st]),
    "dsx_lpips_frames": (_i, [_hn, _Df, _Df, _i, _i, _i, _i, _i, _i, _Df, _st]),
    "dsx_lpips_layers": (_i, [_hn, C.POINTER(LpipsLayerTable)]),
    "dsx_lpips_copy_workspace": (_i, [_hn, _u64, C.c_size_t, _Dv, _st]),
    "dsx_resize_coeffs": (_i, [_i, _i, _i, _pi32, _pi32, _pi32, _i]),
    "dsx_resize_plan_create": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "dsx_resize_plan_destroy": (None, [_hn]),
    "dsx_resize_workspace_bytes": (C.c_size_t, [_hn, _i]),
    "dsx_resize_u8": (_i, [_hn, _D8, _i, _D8, _D8, _st]),
    "dsx_u8_to_tensor": (_i, [_D8, _i, _i, _i, _i, _f, _f, _Df, _st]),
    "dsx_tileplan_create": (_i, [_pi64, _pi64, _pi64, _i, C.POINTER(_vp)]),
    "dsx_tileplan_destroy": (None, [_hn]),
    "dsx_tileplan_total": (_i64, [_hn]),
    "dsx_tileplan_regions": (_i, [_hn, _pi32, _i64]),
    "dsx_tileplan_gather": (_i, [_hn, _Df, _i64, _i64, _i64, _Df, _st]),
    "dsx_tileplan_gather_norm": (_i, [_hn, _Df, _Df, _i64, _i64, _i64, _f, _f, C.POINTER(C.c_double), _i, _Df, _Df, _st]),
    "dsx_tileplan_gather_mix": (_i, [_hn, _Df, _Df, _i64, _i64, _i64, C.POINTER(C.c_double), C.c_double,
                                     C.POINTER(C.c_double), _Df, _Df, _Df, _st]),
    "dsx_tileplan_gather_input": (_i, [_hn, _Dv, _i, _i64, _i64, _i64, C.c_double, C.c_double, C.c_double, _Df, _st]),
    "dsx_tileplan_randn": (_i, [_hn, _i, _i64, _i64, _i64, _u64, _u64, C.c_uint32, _Df, _st]),
    "dsx_moments_update": (_i, [_Df, _Dd, _Dd, _i64, _i, _st]),
    "dsx_moments_finish": (_i, [_Dd, _Dd, _i64, _i, _Df, _Df, _st]),
    "dsx_tileplan_stitch": (_i, [_hn, _Df, _i, _i64, _i64, _i64, _Df, _Df, _Dd, _st]),
    "dsx_tileplan_pack_layout": (_i, [_hn, _i, _pi64, _pi64]),
    "dsx_tileplan_pack": (_i, [_hn, _Df, _i, _i, _i64, _i64, _Df, _st]),
    "dsx_tileplan_paste_packed": (_i, [_hn, _Df, _i, _i, _i64, _Df, _Df, _Dd, _st]),
    "dsx_tileplan_contributors": (_i, [_hn, _pi32, _pi32]),
    "dsx_tileplan_set_window": (_i, [_hn, _H, _H]),
    "dsx_tileplan_blend_blocks": (_i, [_hn]),
    "dsx_tileplan_blend": (_i, [_hn, _Df, _i, _i, _i64, _Df, _Df, _Dd, _st]),
    "dsx_tileplan_gather_canvas": (_i, [_hn, _Df, _i, _i64, _i64, _i64, _Df, _st]),
    "dsx_tileplan_blend_step": (_i, [_hn, _Df, _i, _i, _i64, _Df, _f, _f, _f, _u64, _u64, C.c_uint32, _st]),
    "dsx_tileplan_crop_lines": (_i, [_hn, _i, _H, _H]),
    "dsx_tileplan_disagreement": (_i, [_hn, _Df, _i, _i, _i64, _i, _Df, _Dd, _st]),
    "dsx_tiff_open": (_i, [C.c_char_p, C.POINTER(_vp)]),
    "dsx_tiff_info": (_i, [_hn, _pi64, C.POINTER(_i)]),
    "dsx_tiff_read": (_i, [_hn, _i64, _i64, _H, C.c_size_t]),
    "dsx_tiff_close": (None, [_hn]),
    "dsx_tiff_write": (_i, [C.c_char_p, _H, _i64, _i64, _i64, _i, C.c_char_p, _i]),
    "dsx_frames_to_f32": (_i, [_Dv, _i, _i64, C.c_double, _Df, _st]),
    "dsx_order_stats_workspace_bytes": (C.c_size_t, [_i64, _i]),
    "dsx_order_stats": (_i, [_Df, _Df, _i64, C.c_double, C.c_double, _pi64, _i, C.POINTER(C.c_double), _Dv, _st]),
    "dsx_comoments_blocks": (_i, [_i64]),
    "dsx_comoments": (_i, [_Df, _Df, _Df, _i64, _i64, _pi64, _Dd, _Dd, _st]),
    "dsx_calibration_blocks": (_i, [_i64]),
    "dsx_calibration": (_i, [_Df, _Df, _Df, _i64, _i, _H, _i, _H, _i, _Dd, _Dd, _st]),
    "dsx_sample_quantiles": (_i, [_Df, _i64, _i, _i64, _H, _i, _Df, _Df, _Df, _st]),
    "dsx_consistency_blocks": (_i, [_i64]),
    "dsx_consistency": (_i, [_Dv, _i, _Df, _Df, _i64, _i64, _i, _H, _H, _H, C.c_double, C.c_double, _Df, _Df, _Df, _Dd, _Dd,
                             _st]),
}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). There is no CPU fallback for the sampling path.")


def _host_address(a, where):
    if isinstance(a, np.ndarray) and a.flags.c_contiguous:
        return a.ctypes.data
    if isinstance(a, torch.Tensor) and a.device.type == "cpu" and a.is_contiguous():
        return a.data_ptr()
    if isinstance(a, (np.ndarray, torch.Tensor)):
        raise DsxError(f"{where} takes host memory as it lies: a C-contiguous numpy array or a contiguous CPU tensor")
    return a                                        # None, an address, a ctypes object: ctypes converts those


def host_pointers(tensors):
    """The addresses of contiguous CPU tensors as a ``void*[]`` (the caller keeps the tensors alive)."""
    return (C.c_void_p * len(tensors))(*[_host_address(t, "a host pointer array") for t in tensors])


def plane_view(t, where):
    """(address, planes, n, plane stride, pixel stride) of a CUDA fp32 tensor (planes, ...) read IN PLACE by a call that
    takes {plane, pixel} element strides (dsx_comoments): the dimensions behind the first must collapse into one
    stride, as they do for a contiguous tensor, a channel of a (b, C, p, p) tensor or a channel of a channel-last
    canvas.  The address goes into a Dev slot as it is; the call's contiguous tensors name its device."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() < 2:
        got = f"{t.dtype} on {t.device}, {t.dim()} dimensions" if isinstance(t, torch.Tensor) else type(t).__name__
        raise DsxError(f"{where} must be a CUDA float32 tensor (planes, ...), got {got}")
    dims = [(n, s) for n, s in zip(t.shape[1:], t.stride()[1:]) if n != 1]
    n = 1
    for size, _ in dims:
        n *= size
    if n < 1 or any(s < 1 for _, s in dims) or any(dims[k][1] != dims[k + 1][0] * dims[k + 1][1] for k in range(len(dims) - 1)):
        raise DsxError(f"{where}: shape {tuple(t.shape)} with strides {t.stride()} is no stack of planes with one pixel "
                       "stride; pass a contiguous copy")
    pixel = dims[-1][1] if dims else 1
    plane = t.stride(0) if t.shape[0] > 1 else (n - 1) * pixel + 1
    return t.data_ptr(), int(t.shape[0]), int(n), int(plane), int(pixel)


def stack_view(t, where):
    """(address, n, count, sample stride) of a CUDA fp32 tensor (n, ...) read IN PLACE as n samples of ``count`` contiguous
    elements, one every ``stride`` elements (dsx_sample_quantiles): the whole of a contiguous tensor, or a view such as
    ``buf[:, :b]`` whose first stride exceeds a sample's size.  The address goes into a Dev slot as it is; the call's
    contiguous tensors name its device."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DsxError(f"{where} must be a CUDA tensor: the quantiles run on the MI355X only (no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() < 2 or t.numel() < 1:
        raise DsxError(f"{where} must be a non-empty float32 tensor (n, ...), got {t.dtype} {tuple(t.shape)}")
    count = t[0].numel()
    stride = int(t.stride(0)) if t.shape[0] > 1 else count
    if not t[0].is_contiguous() or stride < count:
        raise DsxError(f"{where} must hold contiguous samples, one every stride >= their size: shape {tuple(t.shape)} with "
                       f"strides {t.stride()}; pass a contiguous copy")
    return t.data_ptr(), int(t.shape[0]), int(count), stride


def common_device(name, devices):
    """The device a call runs on: the one device of all its tensors, None without a tensor; two devices are refused."""
    for d in devices[1:]:
        if d != devices[0]:
            raise DsxError(f"{name}: tensors on {devices[0]} and on {d}; a call runs on one device")
    return devices[0] if devices else None


def bind(name, fn, kinds):
    """The Python callable of one entry: ``fn`` (the C function, or a stand-in) behind the conversions ``kinds`` ask for.
    Tensors in Dev slots are checked and name the call's device: the call runs under it, and a None stream is its
    current stream.  Without a tensor nothing is guarded and None stays NULL.  ``fn``'s value is returned as it is."""
    dev_slots = [(i, k.elem, DEV_DTYPES[k.elem]) for i, k in enumerate(kinds) if isinstance(k, _Kind) and k.name == "Dev"]
    host_slots = [i for i, k in enumerate(kinds) if k == Host]
    stream_slot = kinds.index(Stream) if Stream in kinds else None
    if not dev_slots and not host_slots and stream_slot is None:
        return fn                                   # scalars, handles, typed host pointers: ctypes converts those

    def call(*args):
        if len(args) != len(kinds):
            raise TypeError(f"{name} takes {len(kinds)} arguments, got {len(args)}")
        args, devices = list(args), []
        for i, elem, dtypes in dev_slots:
            a = args[i]
            if isinstance(a, torch.Tensor):
                if not a.is_cuda or not a.is_contiguous() or (dtypes is not None and a.dtype not in dtypes):
                    raise DsxError(f"{name}: argument {i} must be a contiguous CUDA tensor of {elem}, got {a.dtype} "
                                   f"on {a.device}{'' if a.is_contiguous() else ', strided'}")
                devices.append(a.device)
                args[i] = a.data_ptr()
        for i in host_slots:
            args[i] = _host_address(args[i], f"{name}: argument {i}")
        dev = common_device(name, devices)
        if stream_slot is not None:
            s = args[stream_slot]
            if isinstance(s, torch.cuda.Stream):
                args[stream_slot] = s.cuda_stream
            elif s is None and dev is not None:
                args[stream_slot] = torch.cuda.current_stream(dev).cuda_stream
        if dev is None:
            return fn(*args)
        with torch.cuda.device(dev):
            return fn(*args)
    return call


_cdll = C.CDLL(LIB_PATH)
lib = types.SimpleNamespace()                       # lib.dsx_*: every entry of SIGNATURES, bound once
for _name, (_res, _kinds) in SIGNATURES.items():
    if not hasattr(_cdll, _name):
        if "DSX_LIB_PATH" not in os.environ:
            getattr(_cdll, _name)      # raises: the product library must export everything include/dsx.h declares
        # a diagnostic variant (tools/build_variant.sh) built before an entry point was added: usable for timing
        # experiments, the missing call fails loudly if it is ever made
        def _missing(*_a, _n=_name, **_k):
            raise DsxError(f"{LIB_PATH} (DSX_LIB_PATH variant) does not export {_n}: rebuild the variant")
        setattr(lib, _name, _missing)
        continue
    _fn = getattr(_cdll, _name)
    _fn.restype = _res
    _fn.argtypes = [k.ctype if isinstance(k, _Kind) else k for k in _kinds]
    setattr(lib, _name, bind(_name, _fn, _kinds))


def check(rc):
    """Raise DsxError with the library's message on a negative status."""
    if rc is not None and rc < 0:
        raise DsxError(f"libdsx status {rc}: {lib.dsx_last_error().decode(errors='replace')}")
    return rc


def require_gpu():
    if lib.dsx_device_count() < 1:
        raise DsxError("no HIP device visible: the sampling path runs on MI355X only (no CPU fallback)")
