import sys, os, torch
sys.path.insert(0, os.getcwd())
import bench
from diffsplitting_amd import engine
torch.set_grad_enabled(False)
if len(sys.argv) > 2 and sys.argv[1] == "dump-img-model":
    # python tools/determinism_check.py dump-img-model DIR: one forward of the smallest model whose 8 x 8 level reaches every
    # k_conv_img instantiation (tests/test_conv_img_plan_cpu.py), B = 3, in every operand type -> DIR/img_model_<type>.npy.
    # Run it once per library (DSX_LIB_PATH) and compare the files with np.array_equal: a bitwise A/B that covers f16.
    import numpy as np
    kw = dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=(1, 4, 8), attn_res=(8,), res_blocks=1, image_size=32)
    os.makedirs(sys.argv[2], exist_ok=True)
    for dtype in ("bf16", "f16", "f32"):
        eng = engine.UNetEngine(engine.make_cfg("sr3", **kw), "sr3")
        eng.load_state_dict(bench.random_init_state_dict(eng.param_names, eng.param_shapes, seed=11)); eng.finalize(dtype)
        g = torch.Generator().manual_seed(77)
        x = torch.randn(3, 6, 32, 32, generator=g).cuda(); t = (0.05 + 0.9 * torch.rand(3, 1, generator=g)).cuda()
        y = eng.forward(x, t, cond_channels=3).float().cpu().numpy()
        np.save(os.path.join(sys.argv[2], "img_model_%s.npy" % dtype), y)
        print(dtype, "img model forward dumped, finite:", bool(np.isfinite(y).all()))
        del eng
    sys.exit(0)
cfg = engine.make_cfg("sr3", **{k: bench.UNET[k] for k in ("in_channel", "out_channel", "inner_channel", "norm_groups", "channel_mults", "attn_res", "res_blocks", "image_size")})
for dtype in ("bf16", "f32"):
    eng = engine.UNetEngine(cfg, "sr3")
    eng.load_state_dict(bench.random_init_state_dict(eng.param_names, eng.param_shapes)); eng.finalize(dtype)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, 6, 128, 128, generator=g).cuda(); t = (0.05 + 0.9 * torch.rand(16, 1, generator=g)).cuda()
    ref = eng.forward(x, t, cond_channels=3).clone()
    bad = 0
    for i in range(30):
        y = eng.forward(x, t, cond_channels=3)
        if not torch.equal(y, ref): bad += 1
    print(dtype, "forward B=16 x30 bitwise mismatches:", bad, "finite:", bool(torch.isfinite(ref).all()))
    # sampling loop determinism (graph), 40 steps, twice
    bufs, gam = engine.gaussian_buffers(bench.SCHEDULE)
    full = engine.gaussian_step_table(bufs, gam, "sr3", clip_denoised=True)
    import numpy as np
    idx = np.arange(40)
    tab = engine.StepTableHost(full.tcond[idx], c1=full.c1[idx], c2=full.c2[idx], sigma=full.sigma[idx], a=full.a[idx], b=full.b[idx], predict_eps=True, clip=True)
    cond = x[:, :3].contiguous(); x0 = engine.randn((16, 3, 128, 128), seed=5)
    o1 = eng.sample_loop(tab, x0.clone(), cond=cond, seed=7)[0].clone()
    o2 = eng.sample_loop(tab, x0.clone(), cond=cond, seed=7)[0].clone()
    print(dtype, "40-step loop bitwise equal:", bool(torch.equal(o1, o2)))
    del eng
