"""The plans and case tables that a GPU test runs and a CPU test pins against the planner's dry run (tests/direct_cases.py
holds those of the direct rows): the planner's configurations and knob settings, the plans off the 8 x 8 tile grid, the
plans with GroupNorm groups wider than 64 channels, and the model whose 8 x 8 level takes the image-resident kernel."""
import json
import os

from oracle import cases

DT = ("bf16", "f16", "f32")      # the operand types, in the order of tests/layer_check.py's DT (no torch needed here)

# ----------------------------------------------------------------------------- tests/test_planner_cpu.py, tools/plan_dumps.py
# (flavour, cfg kwargs, B, H, W, cond_channels)
CONFIGS = {
    "c2_sr3_128_b16": ("sr3", dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32,
                                   channel_mults=(1, 2, 4, 8, 8), attn_res=(16,), res_blocks=2, image_size=128), 16, 128, 128, 3),
    "c2_sr3_128_b1": ("sr3", dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32,
                                  channel_mults=(1, 2, 4, 8, 8), attn_res=(16,), res_blocks=2, image_size=128), 1, 128, 128, 3),
    "c4_sr3_512_b2": ("sr3", dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=16,
                                  channel_mults=(1, 2, 4, 8, 16), attn_res=(), res_blocks=1, image_size=512), 2, 512, 512, 3),
    "c3_hagen_512_b8": ("ddpm", dict(in_channel=2, out_channel=2, inner_channel=16, norm_groups=16,
                                     channel_mults=(1, 2, 4, 8), attn_res=(), res_blocks=1, image_size=32), 8, 512, 512, 0),
    "c1_cifar_32_b4": ("ddpm", dict(in_channel=6, out_channel=6, inner_channel=16, norm_groups=16,
                                    channel_mults=(1, 2, 4, 8), attn_res=(), res_blocks=1, image_size=32), 4, 32, 32, 0),
    "ragged_48x80_b3": ("ddpm", dict(in_channel=2, out_channel=2, inner_channel=16, norm_groups=16,
                                     channel_mults=(1, 2, 4), attn_res=(), res_blocks=1, image_size=32), 3, 48, 80, 0),
}

# the settings of the round-1 tuning sweeps (tools/tune.sh runs), the faulting one first
ENV_SETS = [
    {"DSX_MIN_GRID": "448"},
    {},
    {"DSX_MIN_GRID": "256"}, {"DSX_MIN_GRID": "384"}, {"DSX_MIN_GRID": "768"}, {"DSX_MIN_GRID": "1024"}, {"DSX_MIN_GRID": "2048"},
    {"DSX_WS_MIN_GRID": "1"}, {"DSX_WS_MIN_GRID": "448"}, {"DSX_WS_MIN_GRID": "100000"},
    {"DSX_WS": "0"}, {"DSX_SPLITK": "0"}, {"DSX_FUSE_STATS": "0"}, {"DSX_WS": "0", "DSX_SPLITK": "0", "DSX_FUSE_STATS": "0"},
    {"DSX_TILES_WIDE": "1,2,5"}, {"DSX_TILES_WIDE": "0,1,2,5"}, {"DSX_TILES_WIDE": "2,5"}, {"DSX_TILES_NARROW": "4,5"},
    {"DSX_TILES_NARROW": "3,4,5"}, {"DSX_TILES_WIDE_SPLIT": "1,2,5"}, {"DSX_TILES_NARROW_SPLIT": "4,5"},
    {"DSX_TILES_WS_WIDE": "2"}, {"DSX_TILES_WS_WIDE": "2,1"}, {"DSX_TILES_WS_WIDE_1X1": "2"}, {"DSX_TILES_WS_NARROW": "5"},
    {"DSX_TILES_WS_NARROW": "5,4"}, {"DSX_MIN_GRID": "448", "DSX_TILES_WIDE": "0,2,3,4"}, {"DSX_MIN_GRID": "448", "DSX_WS": "0"},
    # round 3: chunks per item of the persistent kernel, the 1 x 1 XCD mapping
    {"DSX_WS_G2": "0"}, {"DSX_WS_C4": "0"}, {"DSX_WS_MAP3": "0"}, {"DSX_WS_G2": "0", "DSX_WS_C4": "0", "DSX_WS_MAP3": "0"},
    {"DSX_WS_G4_MIN64": "1000"}, {"DSX_WS_G2_MIN64": "2", "DSX_WS_G2_MIN128": "2", "DSX_WS_G4_MIN64": "4", "DSX_WS_C4_MIN": "4"},
    {"DSX_WS_MIN_GRID": "1", "DSX_WS_G2_MIN64": "2", "DSX_WS_G4_MIN64": "4", "DSX_WS_C4_MIN": "4"},
]


# ----------------------------------------------------------------------------- tests/test_gpu_shapes.py
# any grid fills the chip and the persistent kernel is off: the 128-pixel tiles, two and four images per tile
_SHAPE_WIDE_TILES = {"DSX_MIN_GRID": "1", "DSX_WS": "0"}
_SHAPE_MANY_CHUNKS = {"DSX_WS_MIN_GRID": "1", "DSX_WS_G2_MIN64": "2", "DSX_WS_G2_MIN128": "2", "DSX_WS_G4_MIN64": "4",
                "DSX_WS_C4_MIN": "4"}        # as in tests/test_gpu_layers.py: k_conv_ws on the 128-pixel tile
_SHAPE_SPLITK = {"DSX_MIN_GRID": "100000", "DSX_WS": "0"}

# id -> (case, dtype, B, env)
SHAPE_PLANS = {}
for _c in cases.SHAPE_CASES:
    for _d in DT:
        SHAPE_PLANS[f"{_c}_{_d}"] = (_c, _d, 3, {})
for _c, _v in cases.SHAPE_CASES.items():
    if _v["model"] in ("sr3_tiny", "w20"):
        for _d in DT:
            SHAPE_PLANS[f"{_c}_{_d}_wide_tiles"] = (_c, _d, 3, _SHAPE_WIDE_TILES)
# (ddpm_tiny's 32-channel level on the slim 128 x 32 tile: the only plain 3 x 3 launches at 4x32x1 and 16x4x2 -- in
# sr3_tiny and w20 that level is wider than 32 channels and takes the 64-pixel tile first)
for _s in ("128x24", "24x64"):
    for _d in DT:
        SHAPE_PLANS[f"ddpm_tiny_{_s}_{_d}_wide_tiles"] = (f"ddpm_tiny_{_s}", _d, 3, _SHAPE_WIDE_TILES)
for _m in ("ddpm_tiny", "sr3_tiny"):
    for _s in ("64x48", "64x24", "128x24"):
        for _d in DT:
            SHAPE_PLANS[f"{_m}_{_s}_{_d}_many_chunk_ws"] = (f"{_m}_{_s}", _d, 3, _SHAPE_MANY_CHUNKS)
for _h, _w in cases.SHAPE_SIZES:
    SHAPE_PLANS[f"sr3_tiny_{_h}x{_w}_f32_splitk"] = (f"sr3_tiny_{_h}x{_w}", "f32", 3, _SHAPE_SPLITK)   # stride 2 under split-K
# one image on two-image tiles (2x16x2 on the 16 x 6 maps): half of every such tile is empty
SHAPE_PLANS["ddpm_tiny_64x24_b1_bf16"] = ("ddpm_tiny_64x24", "bf16", 1, {})
SHAPE_PLANS["ddpm_tiny_64x24_b1_f32"] = ("ddpm_tiny_64x24", "f32", 1, {})

# The geometry classes (tests/layer_check.py geom_tag, less its +tail suffix) that the union over the operand types must
# contain.  What each operand type must contain is REACH_BY_DTYPE, which tests/test_planner_cpu.py holds equal to what
# the planner's dry run of these very plans gives.
_NARROW5 = ("2x16x2", "2x32x1", "4x16x1", "8x4x2", "16x2x2")


def _classes(fam, size, tiles, bm):
    return {f"{fam} {size} {t}@{bm}" for t in tiles}


SHAPE_REACH = (_classes("mfma", "1x1", _NARROW5, 64)
         | _classes("mfma", "1x1", ("2x16x4", "2x32x2", "4x16x2", "4x32x1", "8x4x4", "16x2x4", "16x4x2"), 128)
         | _classes("mfma", "3x3", _NARROW5, 64) | _classes("mfma", "3x3", ("4x16x2", "4x32x1", "16x4x2"), 128)
         | _classes("mfma", "3x3 up", ("4x16x1",), 64) | _classes("mfma", "3x3 up", ("4x32x1", "16x4x2"), 128)
         | _classes("mfma", "3x3 s2", _NARROW5, 64)
         | _classes("g2", "3x3", ("4x32x1", "16x8x1"), 128)
         | _classes("splitK", "1x1", _NARROW5, 64) | _classes("splitK", "3x3", _NARROW5, 64)
         | _classes("splitK", "3x3 up", ("4x16x1",), 64) | _classes("splitK", "3x3 s2", _NARROW5, 64)
         | _classes("ws", "1x1", ("2x32x1", "4x16x1"), 64) | _classes("ws", "1x1", ("4x32x1", "8x16x1"), 128)
         | _classes("ws", "3x3", ("4x16x1",), 64) | _classes("ws", "3x3", ("8x16x1",), 128)
         | _classes("ws", "3x3 up", ("4x16x1",), 64))
# multi-image tiles whose last tile misses images (B = 3 on two- and four-image tiles), with their suffix
SHAPE_REACH_TAILS = ({c + "+tail" for c in _classes("mfma", "3x3", ("8x4x2", "2x16x2", "16x2x2"), 64)}
               | {c + "+tail" for c in _classes("mfma", "1x1", ("2x16x4", "2x32x2", "4x16x2", "8x4x4", "16x2x4", "16x4x2"),
                                                128)})


def shape_reach_by_dtype():
    """dtype -> the classes its plans must reach (tests/golden/shape_reach.json): tests/test_planner_cpu.py asserts that
    this equals what the planner's dry run of SHAPE_PLANS gives, so the table cannot drift from the planner unnoticed"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_reach.json")) as f:
        return {d: set(v) for d, v in json.load(f).items()}


# ----------------------------------------------------------------------------- tests/test_gpu_groups.py
# k_conv_ws wherever it fits (g2: its 16 x 16 level on the persistent kernel, three hosted finalizes of 128 channels per
# group, k_gn_finalize launches with four partial rows); no hosted finalize (the same GroupNorms by launches of their own)
_GROUP_WS = {"DSX_WS_MIN_GRID": "1"}
_GROUP_NO_HOST = {"DSX_HOST_FIN": "0"}
# any grid fills the chip and the persistent kernel is off: other tiles, so other partial-row counts per source
_GROUP_WIDE_TILES = {"DSX_MIN_GRID": "1", "DSX_WS": "0"}

# id -> (case, dtype, env, flat).  Every case in every operand type at default knobs; a flat plan per case in f32 and bf16.
GROUP_PLANS = {}
for _c in cases.GROUP_CASES:
    for _d in ("bf16", "f16", "f32"):
        GROUP_PLANS[f"{_c}_{_d}"] = (_c, _d, {}, False)
    for _d in ("f32", "bf16"):
        GROUP_PLANS[f"{_c}_{_d}_flat"] = (_c, _d, {}, True)
GROUP_PLANS["g2_bf16_ws"] = ("g2", "bf16", _GROUP_WS, False)
GROUP_PLANS["g2_f32_ws"] = ("g2", "f32", _GROUP_WS, False)
GROUP_PLANS["g1_f16_no_host"] = ("g1", "f16", _GROUP_NO_HOST, False)
GROUP_PLANS["g1_bf16_wide_tiles"] = ("g1", "bf16", _GROUP_WIDE_TILES, False)

# What must have been checked, per operand type, after every plan ran (test_reach; layer_check.group_reach_tags derives
# them from the dumped launches).
GROUP_REACH = ("fin>64", "wide own>64", "wide>256", "hosted>64", "straddle>64", "f32part>64", "shifted>64", "8x8 no img",
         "npow2>64")
GROUP_REACH_EXEMPT = {}      # dtype -> {tag: reason}: every operand type reaches every tag (g1 at default knobs alone does)


# ----------------------------------------------------------------------------- tests/test_gpu_conv_img.py
# SR3 UNet: 32 x 32 input, levels 64 / 256 / 512 channels, attention at 8 x 8, 3 conditioning channels
IMG_MODEL = dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=(1, 4, 8),
                 attn_res=(8,), res_blocks=1, image_size=32)
COND_CHANNELS = 3

IMG_LAUNCHES = {
    "conv3x3 256->512 @8x8 img": 1,
    "conv1x1 256->512 @8x8 img": 1,
    "conv3x3 512->512 @8x8 img": 7,
    "conv1x1 512->1536 @8x8 img": 4,
    "conv1x1 512->512 @8x8 img": 4,
    "conv3x3 1024->512 @8x8 img": 1,
    "conv1x1 1024->512 @8x8 img": 1,
    "conv1x1 768->512 @8x8 img": 1,
}
