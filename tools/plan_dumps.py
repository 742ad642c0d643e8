"""Dump the dry-run plan (DSX_PLAN_DUMP) of every entry of CONFIGS x {f32, bf16, f16} x ENV_SETS of
tests/test_planner_cpu.py and print the number of dumps and one sha256 over all of them.  Two builds of the library plan
alike exactly when the figures agree (DSX_LIB_PATH selects the library; `cmp` the files to find a difference).

    python tools/plan_dumps.py OUTDIR"""
import ctypes as C, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.plan_cases import CONFIGS, ENV_SETS
from diffsplitting_amd import _lib
out = sys.argv[1]
os.makedirs(out, exist_ok=True)
all_keys = {k for e in ENV_SETS for k in e}
h = hashlib.sha256()
n = 0
for ei, env in enumerate(ENV_SETS):
    for k in all_keys: os.environ.pop(k, None)
    os.environ.update(env)
    for name, (flavour, kw, B, H, W, cc) in CONFIGS.items():
        cfg = _lib.UnetCfg()
        cfg.flavour = 0 if flavour == "sr3" else 1
        for k in ("in_channel", "out_channel", "inner_channel", "norm_groups", "res_blocks", "image_size"):
            setattr(cfg, k, kw[k])
        cfg.n_mults = len(kw["channel_mults"]); cfg.n_attn_res = len(kw["attn_res"]); cfg.with_time_emb = 1
        for i, m in enumerate(kw["channel_mults"]): cfg.channel_mults[i] = m
        for i, m in enumerate(kw["attn_res"]): cfg.attn_res[i] = m
        for dt, code in (("f32", 0), ("bf16", 1), ("f16", 2)):
            path = os.path.join(out, f"{ei:02d}_{name}_{dt}.txt")
            os.environ["DSX_PLAN_DUMP"] = path
            a, b, l = C.c_size_t(), C.c_size_t(), C.c_int()
            _lib.check(_lib.lib.dsx_plan_dry_run(C.byref(cfg), code, B, H, W, cc, C.byref(a), C.byref(b), C.byref(l)))
            data = open(path, "rb").read()
            assert data.count(b"\n") > 10, path
            h.update(data); n += 1
print(n, h.hexdigest())
