"""Reading a DSX_PLAN_DUMP file (planner dry run: no GPU, no compute): one line per launch, with the launch's argument
struct as hex bytes.  Shared by the CPU tests that pin what a GPU module covers (tests/test_conv_img_plan_cpu.py for
k_conv_img, tests/test_planner_cpu.py for the tile geometries of tests/test_gpu_shapes.py, tests/test_groups_plan_cpu.py
for the GroupNorm finalizes of tests/test_gpu_groups.py)."""
import ctypes as C
import re


class ConvArgsHead(C.Structure):
    """the leading members of ConvArgs (dsx_kernels.h), up to the ones read here: DSX_PLAN_DUMP writes the struct's bytes"""
    _fields_ = [("src0", C.c_void_p), ("src1", C.c_void_p), ("act_bf16", C.c_int), ("out_bf16", C.c_int),
                ("C0", C.c_int), ("C1", C.c_int), ("B", C.c_int), ("Hs", C.c_int), ("Ws", C.c_int), ("up", C.c_int),
                ("Ho", C.c_int), ("Wo", C.c_int), ("gn_scale", C.c_void_p), ("gn_shift", C.c_void_p),
                ("has_gn", C.c_int), ("swish", C.c_int), ("stage_mode", C.c_int), ("wpack", C.c_void_p),
                ("bias", C.c_void_p), ("film", C.c_void_p), ("film_bs", C.c_int), ("resid", C.c_void_p),
                ("resid_ld", C.c_int), ("out", C.c_void_p), ("out_ld", C.c_int), ("Cout", C.c_int),
                ("nblocks", C.c_int), ("kchunks", C.c_int), ("tw_log2", C.c_int), ("th_log2", C.c_int),
                ("tb_log2", C.c_int), ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("m_tiles", C.c_int),
                ("n_tiles", C.c_int), ("lds_row", C.c_int), ("cpg", C.c_int), ("ws_wg_per_n", C.c_int),
                ("ws_cpg", C.c_int), ("xcd_bands", C.c_int), ("ws_map", C.c_int), ("ws_nt_log2", C.c_int),
                ("ws_per", C.c_int), ("ws_adv_x", C.c_int), ("ws_adv_y", C.c_int), ("ws_adv_b", C.c_int),
                ("ws_dpy", C.c_int), ("ws_dpx", C.c_int), ("mg_tiles_x", C.c_uint), ("mg_per_img", C.c_uint),
                ("mg_pw", C.c_uint), ("mg_wpn", C.c_uint), ("mg_per", C.c_uint), ("ws_bigdiv", C.c_int),
                ("stat_part", C.c_void_p)]


class StatPivot(C.Structure):
    _fields_ = [("bias", C.c_void_p), ("film", C.c_void_p), ("film_bs", C.c_int)]


class GnFinArgsHead(C.Structure):
    """the leading members of GnFinArgs (dsx_kernels.h), up to `count`"""
    _fields_ = [("part0", C.c_void_p), ("C0", C.c_int), ("nchunk0", C.c_int), ("f32_0", C.c_int),
                ("part1", C.c_void_p), ("C1", C.c_int), ("nchunk1", C.c_int), ("f32_1", C.c_int),
                ("piv0", StatPivot), ("piv1", StatPivot), ("B", C.c_int), ("groups", C.c_int), ("count", C.c_double)]


_LINE = re.compile(r'(\d+) kind=(\d+) desc="([^"]*)" flops=\S+ bytes=\S+ launcher=(\w+) dtype=(\d+) tile=(-?\d+) '
                   r'ks=(\d+) stride=(\d+) col_split=\d+ args=([0-9a-f]+)$')
CONV_LAUNCHERS = ("conv_first", "conv_img", "conv_mfma", "conv_ws")     # their args begin with a ConvArgs
# a finalize launch of its own, named by the kernel its launch rule picks (gn_finalize_is_wide); args: a GnFinArgs
FIN_LAUNCHERS = ("gn_finalize", "gn_finalize_wide")


def read_dump(path):
    """[dict(index, kind, desc, launcher, dtype, tile, ks, stride, raw, conv, fin)] of a dump, in launch order; `conv` is
    the ConvArgsHead of a launch whose arguments begin with a ConvArgs, `fin` the GnFinArgsHead of a finalize launch,
    else None"""
    out = []
    with open(path) as f:
        lines = f.read().splitlines()
    for i, line in enumerate(lines):
        m = _LINE.match(line)
        assert m and int(m.group(1)) == i, line[:200]
        raw = bytes.fromhex(m.group(9))
        conv = None
        if m.group(4) in CONV_LAUNCHERS:
            assert len(raw) >= C.sizeof(ConvArgsHead), line[:200]
            conv = ConvArgsHead.from_buffer_copy(raw[:C.sizeof(ConvArgsHead)])
        fin = None
        if m.group(4) in FIN_LAUNCHERS:
            assert len(raw) >= C.sizeof(GnFinArgsHead), line[:200]
            fin = GnFinArgsHead.from_buffer_copy(raw[:C.sizeof(GnFinArgsHead)])
        out.append(dict(index=i, kind=int(m.group(2)), desc=m.group(3), launcher=m.group(4), dtype=int(m.group(5)),
                        tile=int(m.group(6)), ks=int(m.group(7)), stride=int(m.group(8)), raw=raw, conv=conv, fin=fin))
    return out
