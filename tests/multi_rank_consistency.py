"""Child program of test_gpu_consistency (one process per rank): every rank runs
predict_stack(samples=2, return_std=True, seed=11, consistency="project") on an input-only uint16 stack with an input
clip -- its share of the tiles, two collectives (one per canvas), then the consistency pass on the stitched canvases,
which every rank holds -- and checks the projected canvases, the kept raw mean and the report rows, bitwise, against
core.consistency.consistency applied to the one-rank canvases restated in this process (every tile id, no collective,
the same batches of two)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 11


def main():
    from diffsplitting_amd import engine
    from diffsplitting_amd.core.consistency import consistency
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_stack
    from diffsplitting_amd.model import networks
    from tests import nets
    from tests.bits import same_bits
    from tests.rank_worker import finish, start
    from tests.util import golden_state_dict
    rank, world = start()
    sd, _ = golden_state_dict("unet_hagen_64")
    netG = networks.define_G(nets.opt(nets.hagen64_section())).cuda()
    netG.load_state_dict({"denoise_fn." + k: v for k, v in sd.items()})
    s = np.random.default_rng(5).integers(0, 6000, (2, 64, 96)).astype(np.uint16)
    nd = dict(mean_input=np.float64(3000.0), std_input=np.float64(1700.0), mean_target=np.array([1500.0, 1400.0]),
              std_target=np.array([850.0, 800.0]), target0_max=None, target1_max=None, input_max=None)
    stack = InputStackTiledPred(s, 64, nd, grid_size=32, input_clip=5000.0)
    plan = stack.plan
    assert plan.total == 4 and plan.total % (2 * world) == 0                         # every batch is full on every rank
    w = (1.0, 0.5)

    got, _ = predict_stack(netG, stack, batch_tiles=2, num_timesteps=2, samples=2, return_std=True, seed=SEED,
                           consistency="project", consistency_noise=2.0, consistency_weights=w)

    means, stds = [], []
    for i in range(0, plan.total, 2):
        chunk = list(range(i, i + 2))
        x = stack.tiles(chunk)["input"]
        mean = m2 = None
        for r in range(2):
            netG.inference(x, continuous=False, num_timesteps=2, seed=SEED, sample_ids=[k + r * plan.total for k in chunk])
            mean, m2 = engine.moments_update(netG.last_full_batch.contiguous(), mean, m2, r)
        m, sd_ = engine.moments_finish(mean, m2, 2)
        means.append(m)
        stds.append(sd_)
    raw_mean, raw_std = plan.stitch(torch.cat(means)), plan.stitch(torch.cat(stds))
    dev, pix, _, clip = stack.acquisition()
    want = consistency(raw_mean, dev, nd, weights=w, std=raw_std, clip=clip, noise=2.0, project=True, pix=pix)

    checks = {"raw": same_bits(got["mean_raw"], raw_mean), "mean": same_bits(got["mean"], want["mean"]),
              "std": same_bits(got["std"], want["std"]),
              "rows": bool(np.array_equal(got["consistency"]["rows"], want["rows"])),
              "moved": not same_bits(got["mean"], raw_mean), "saturated": want["total"]["saturated"] > 0}
    finish(all(checks.values()), "CONSISTENCY", plan.total, world, detail=str(checks))


if __name__ == "__main__":
    main()
