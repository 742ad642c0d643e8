"""In-kernel stamps of one k_conv_img launch, first and last wave of a workgroup side by side (IMG_STAMP in dsx_conv_img.hip):
    DSX_STAMP_OP=<conv ordinal>[,<block>] DSX_LIB_PATH=<-DDSX_STAMPS build> python tools/stamps_img.py
Conv ordinals of the benchmark's plan: 30 conv3x3 512->512, 38 conv3x3 1024->512, 34 conv1x1 512->1536.  Read the shares,
not the length: the stamps' fences and the explicit wait of stamp 16 forbid overlaps the real kernel has."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, numpy as np
import bench
from diffsplitting_amd import engine
from diffsplitting_amd._lib import lib, check
torch.set_grad_enabled(False)
NAMES = {0: "entry", 1: "first loads requested", 19: "GroupNorm arithmetic under way", 2: "scale / shift ready",
         3: "phase 0 converted, up-front loads requested", 18: "first MFMA pair issued", 17: "phase 1 converted",
         16: "last weight fragment landed", 20: "at the reduction barrier", 12: "past the barrier", 13: "partials exchanged",
         14: "reduced and stored", 15: "statistics, end"}
NAMES.update({4 + p: "phase %d MFMAs issued" % p for p in range(8)})
cfg = engine.make_cfg("sr3", **{k: bench.UNET[k] for k in ("in_channel", "out_channel", "inner_channel", "norm_groups", "channel_mults", "attn_res", "res_blocks", "image_size")})
eng = engine.UNetEngine(cfg, "sr3")
eng.load_state_dict(bench.random_init_state_dict(eng.param_names, eng.param_shapes)); eng.finalize(os.environ.get("DT", "bf16"))
ex = eng.executor(16, 128, 128, 3)
n = lib.dsx_exec_num_ops(ex); ms = (C.c_float * n)()
x = torch.randn(16, 6, 128, 128, device="cuda"); t = torch.rand(16, 1, device="cuda")
eng.forward(x, t, cond_channels=3)
check(lib.dsx_exec_profile(ex, 2, ms, None))
buf = (C.c_uint64 * 128)(); check(lib.dsx_exec_read_stamps(ex, buf))
st = np.array(buf[:], dtype=np.int64)
desc = C.create_string_buffer(256); kind = C.c_int(); fl = C.c_double(); by = C.c_double()
want = int(os.environ["DSX_STAMP_OP"].split(",")[0]); k = -1
for i in range(n):
    lib.dsx_exec_op_info(ex, i, desc, 256, C.byref(kind), C.byref(fl), C.byref(by))
    if kind.value == 0:
        k += 1
        if k == want: print("op:", desc.value.decode(), " measured %.1f us" % (ms[i] * 1e3))
t0 = st[0]
print("%-46s %9s %9s" % ("stamp (cycles after wave 0's entry)", "wave 0", "wave 7"))
for i in sorted((i for i in range(32) if st[i] > 0 or st[32 + i] > 0), key=lambda i: st[i] if st[i] > 0 else st[32 + i]):
    f = lambda v: "%9d" % (v - t0) if v > 0 else "%9s" % "-"
    print("%2d %-43s %s %s" % (i, NAMES.get(i, ""), f(st[i]), f(st[32 + i])))
