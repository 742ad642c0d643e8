"""The cases of tests/golden/reduce_bits.npz: every kernel that reduces through csrc/dsx_reduce.h, at the smallest shapes
that give a full chunk, a ragged tail with partly idle waves and more than one workgroup per reduction (stated per
case).  Inputs come from seeded CPU generators; a case returns {output name: array}.  tests/test_gpu_reduce_bits.py
compares them with the recorded bits, tools/gen_reduce_golden.py records them."""
import json

import numpy as np
import torch


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def case_loss():
    """engine.loss_per_sample, L1 and L2: 4366 elements per sample (one full 4096-element chunk and a 270-element tail:
    two workgroups per sample) and 35 elements (less than one wave)."""
    from diffsplitting_amd import engine
    out = {}
    for shape in ((3, 2, 37, 59), (2, 1, 5, 7)):
        a, b = _randn(shape, 101).cuda(), _randn(shape, 102).cuda()
        for name, squared in (("l1", False), ("l2", True)):
            out[f"{name}_{'x'.join(map(str, shape))}"] = engine.loss_per_sample(a, b, squared).cpu().numpy()
    return out


def case_image_metrics():
    """dsx_image_metrics, quantised (uint64 SSD) and not (fp64 SSD): a 35 x 43 valid region = 2 x 2 tiles of 32 x 32,
    the right and bottom ones ragged."""
    from diffsplitting_amd.core import metrics
    a = _randn((2, 3, 45, 53), 111, 0.8)
    b = a + _randn((2, 3, 45, 53), 112, 0.25)
    out = {}
    for name, quantize, rng in (("quantised", True, 255.0), ("float", False, 2.0)):
        ssim, ssd = metrics._run(a.cuda(), b.cuda(), quantize, -1.0, 1.0, rng)
        out[f"{name}_ssim"], out[f"{name}_ssd"] = ssim, ssd
    return out


def case_stitch_psnr():
    """dsx_tileplan_stitch with gt_canvas: frames (2, 40, 56), grid 16, patch 32, two channels -- valid regions from
    16 x 16 to the clipped last row / column, several workgroups per tile with idle lanes in the small regions."""
    from diffsplitting_amd.data.tiling import TilePlan
    plan = TilePlan((2, 40, 56), (1, 16, 16), (1, 32, 32))
    tiles = _randn((plan.total, 2, 32, 32), 121).cuda()
    gt = (_randn((2, 40, 56, 2), 122) * 1.5 + 0.25).cuda()
    canvas = torch.zeros((2, 40, 56, 2), device="cuda")
    part = plan.new_psnr_partials(2, canvas.device)
    plan.stitch_psnr_into(tiles, np.arange(plan.total), canvas, gt, part)
    return {"partials": part.cpu().numpy(), "canvas": canvas.cpu().numpy()}


def case_mix_range():
    """dsx_mix_range: 3000 pixels, n = 10 -- two blocks of eight timesteps (the second ragged), three pixel chunks."""
    from diffsplitting_amd.data.time_predictor_dataset import compute_input_normalization_dict
    g = torch.Generator().manual_seed(131)
    ch = {k: torch.randint(0, 4000, (3000,), generator=g).float().cuda() for k in (0, 1)}
    tab = compute_input_normalization_dict(ch, 10, np.array([759.685, 486.905]), np.array([763.25, 481.5]))
    return {"table": np.array([tab[t] for t in range(11)], dtype=np.float64)}


def case_val_report():
    """dsx_val_report: one input and one target plane of 33 x 67 = 2211 pixels (one ragged workgroup, scalar path)."""
    from diffsplitting_amd.core.validation import validation_report
    g = torch.Generator().manual_seed(141)
    mean, std = 759.685, 486.905
    raw = torch.randint(40, 60000, (1, 1, 33, 67), generator=g).double()
    tar = ((raw - mean) / std).float()
    pred = tar + _randn(tar.shape, 142, 3.0)
    inp = ((raw - 1246.59) / 1246.59).float()
    nd = {"mean_input": np.float64(1246.59), "std_input": np.float64(1246.59), "mean_target": np.array([mean]),
          "std_target": np.array([std])}
    res = validation_report(inp.cuda(), tar.cuda(), pred.cuda(), nd, visuals=False)
    out = {k: getattr(res, k) for k in ("ssd", "tmin", "tmax", "imin", "imax")}
    out["undefined"] = np.array([res.undefined], dtype=np.int64)
    return out


def case_lpips():
    """LPIPS forward on two 64 x 64 pairs (total and the five taps: k_lpips_dist at every channel count), and
    dsx_lpips_frames on one two-channel 64 x 64 frame (k_lpips_minmax: 16 workgroups)."""
    from diffsplitting_amd.core.lpips import LPIPS
    from tests import lpips_ref as R
    model = LPIPS(net='alex', state_dict=R.synth_state_dict()).cuda()
    in0, in1 = R.make_pair(2, 64, 64, 2)
    total, taps = model(in0.cuda(), in1.cuda(), retPerLayer=True)
    tgt, prd = (torch.from_numpy(x).cuda() for x in R.make_frames(shape=(1, 64, 64, 2)))
    return {"total": total.reshape(2).cpu().numpy(), "taps": torch.cat(taps, dim=1).reshape(2, 5).cpu().numpy(),
            "frames_ch0": model.frames(tgt, prd, 0).cpu().numpy(), "frames_ch1": model.frames(tgt, prd, 1).cpu().numpy()}


def case_time_predictor():
    """TimePredictor forward (k_masked_mean) on two 32 x 32 tiles, the network of tests/test_gpu_mixed.py."""
    from diffsplitting_amd.model.ddpm_modules.time_predictor import TimePredictor
    from oracle import cases
    from oracle.weights import synth_state_dict
    from tests.util import load_golden
    keys = [(a, tuple(s)) for a, s in json.loads(bytes(load_golden("refine_n1")["keys_tp"]).decode())]
    tp = TimePredictor(**cases.TIME_PRED_CFG).cuda()
    tp.load_state_dict(synth_state_dict(keys, 0), strict=True)
    return {"t_out": tp(_randn((2, 1, 32, 32), 151).cuda()).reshape(2).cpu().numpy()}


def case_blend_psnr():
    """dsx_tileplan_blend with gt (k_blend's sums): frames (2, 40, 300), grid 16, patch 32 -- 72 tiles, two 256-pixel
    segments per row, the second ragged (44 live lanes: three idle waves and a partly idle one); the "hann" window, so
    the weights are inexact; C = 2 (the wide store) and C = 3."""
    from diffsplitting_amd.data.tiling import TilePlan
    plan = TilePlan((2, 40, 300), (1, 16, 16), (1, 32, 32))
    plan.set_window("hann")
    out = {}
    for Cn in (2, 3):
        tiles = _randn((plan.total, Cn, 32, 32), 160 + Cn).cuda()
        gt = (_randn((2, 40, 300, Cn), 170 + Cn) * 1.5 + 0.25).cuda()
        canvas, _ = plan.blend(tiles, gt=gt)
        out[f"partials_c{Cn}"], out[f"canvas_c{Cn}"] = plan.last_blend_partials.cpu().numpy(), canvas.cpu().numpy()
    return out


def case_stitch_psnr_packed():
    """dsx_tileplan_paste_packed with gt (k_stitch_psnr's packed source): the plan, tiles and gt of case_stitch_psnr,
    the tiles packed for world = 3 into one exchange buffer."""
    from diffsplitting_amd.data.tiling import TilePlan
    plan = TilePlan((2, 40, 56), (1, 16, 16), (1, 32, 32))
    tiles = _randn((plan.total, 2, 32, 32), 121).cuda()
    gt = (_randn((2, 40, 56, 2), 122) * 1.5 + 0.25).cuda()
    world = 3
    flat = torch.zeros((world, plan.rank_stride(world, 2)), device="cuda")
    for q in range(world):
        plan.pack(tiles[q::world], world, q, flat[q])
    canvas, psnr = plan.paste_packed(flat, 2, world, gt=gt)
    return {"canvas": canvas.cpu().numpy(), "psnr": psnr.cpu().numpy()}


def case_msssim():
    """dsx_msssim, five scales, on one (1, 2, 177, 179) pair: 31683 pixels per plane = two statistics chunks, the second
    with a partly idle last pass; range-invariant (k_msssim_stats, k_msssim_coef) and with data_range = 2."""
    from diffsplitting_amd.core.metrics import msssim
    target = _randn((1, 2, 177, 179), 181, 0.8).cuda()
    pred = (0.7 * target.cpu() + _randn((1, 2, 177, 179), 182, 0.3) + 0.4).cuda()
    out = {}
    for name, kw in (("range_invariant", {"range_invariant": True}), ("data_range", {"data_range": 2.0})):
        out[name] = msssim(pred, target, return_scales=True, **kw)[1].numpy()
    return out


def case_comoments():
    """dsx_comoments on three planes: n = 8200 contiguous (the 16-byte path, two workgroups of 4100 pixels per plane,
    the last pass of each with one live thread) and n = 8229 read as channel 1 of a (3, 2, 8229) tensor (the strided
    path, a ragged last group)."""
    from diffsplitting_amd.core.psnr import comoments
    out = {}
    for name, n in (("contiguous", 8200), ("strided", 8229)):
        planes = [(_randn((3, 2, n), 190 + k, 30.0) + 1000.0 * k).cuda() for k in range(3)]
        if name == "contiguous":
            planes = [x[:, 1].contiguous() for x in planes]
        else:
            planes = [x[:, 1] for x in planes]
        out[name] = comoments(*planes).cpu().numpy()
    return out


# fixture key = "<case>/<output>".  Every case runs without autograd (stated here, not by importing this module).
CASES = {"loss": case_loss, "image_metrics": case_image_metrics, "stitch_psnr": case_stitch_psnr,
         "mix_range": case_mix_range, "val_report": case_val_report, "lpips": case_lpips,
         "time_predictor": case_time_predictor, "blend_psnr": case_blend_psnr,
         "stitch_psnr_packed": case_stitch_psnr_packed, "msssim": case_msssim, "comoments": case_comoments}
CASES = {name: torch.no_grad()(case) for name, case in CASES.items()}
