"""The small models of tests/test_gpu_direct.py and what their plans must reach (held on the CPU by
tests/test_direct_plan_cpu.py): the direct rows of k_conv_ws (ConvArgs::ws_direct: plain 1 x 1 convs whose loader waves
DMA the activation units straight into the MFMA images).

A direct row is keyed by (operand type, tile, chunks per item).  Compiled: tile64x128 with two and with four chunks per
item and tile128x64 with two, in every operand type (dsx_conv_variants.h).  DIRECT_ENV forces the persistent kernel and
the four-chunk items onto the small grids of these models (the knobs of tests/test_gpu_layers.py's many-chunk plans)."""
import ctypes as C

from tests.plan_dump import ConvArgsHead

DIRECT_ENV = {"DSX_WS_MIN_GRID": "1", "DSX_WS_G2_MIN64": "2", "DSX_WS_G2_MIN128": "2", "DSX_WS_G4_MIN64": "4",
              "DSX_WS_C4_MIN": "4"}

TILE_64x128, TILE_128x64 = 2, 4                       # ConvTile (dsx_kernels.h)
DIRECT_ROWS = ((TILE_64x128, 2), (TILE_64x128, 4), (TILE_128x64, 2))      # (tile, chunks per item)

# name -> case (flavour, cfg, B, H, W as oracle/cases.py has them) and the operand types it runs in
CASES = {
    # widths 64 / 128 on 32^2 / 16^2 maps, attention at 16^2: every direct row in every operand type; residual convs with
    # one source (fp32: 64 -> 128) and with a concatenated skip (192 -> 128, 256 -> 128, 192 -> 64, 128 -> 64), all
    # hosting a GroupNorm finalize; attention output projections (one source, no finalize)
    "d64": dict(flavour="sr3", B=3, H=32, W=32, dtypes=("bf16", "f16", "f32"),
                cfg=dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=16, channel_mults=(1, 2),
                         attn_res=(16,), res_blocks=1, image_size=32)),
    # K tails: the last item's channel units past Cin exist only as zeros that the buffer descriptor's bounds check
    # supplies.  16-bit: 96 -> 128 in 64-channel items; fp32: 48 -> 128 in 32-channel items (a 16-bit 48-channel conv is
    # one item and never takes the persistent kernel; an fp32 96-channel conv is three whole items)
    "k96": dict(flavour="sr3", B=3, H=32, W=32, dtypes=("bf16", "f16"),
                cfg=dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=8, channel_mults=(3, 4),
                         attn_res=(), res_blocks=1, image_size=32)),
    "k48": dict(flavour="sr3", B=3, H=32, W=32, dtypes=("f32",),
                cfg=dict(in_channel=6, out_channel=3, inner_channel=16, norm_groups=16, channel_mults=(3, 8),
                         attn_res=(), res_blocks=1, image_size=32)),
}
PLANS = [(name, dt) for name, c in CASES.items() for dt in c["dtypes"]]


class ConvArgsDirect(C.Structure):
    """ConvArgs (dsx_kernels.h) up to `ws_direct`, the member behind `stat_part` and `handoff_timeouts`"""
    _fields_ = list(ConvArgsHead._fields_) + [("handoff_timeouts", C.c_void_p), ("ws_direct", C.c_int)]


def direct_flag(op):
    """ConvArgs::ws_direct of a launch read by tests.plan_dump.read_dump (0 for launches that are no conv)"""
    if op["conv"] is None:
        return 0
    return ConvArgsDirect.from_buffer_copy(op["raw"][:C.sizeof(ConvArgsDirect)]).ws_direct


def make_cfg(case):
    from diffsplitting_amd import engine
    cfg = case["cfg"]
    return engine.make_cfg(case["flavour"], cfg["in_channel"], cfg["out_channel"], cfg["inner_channel"],
                           cfg["norm_groups"], cfg["channel_mults"], cfg["attn_res"], cfg["res_blocks"],
                           cfg["image_size"])
