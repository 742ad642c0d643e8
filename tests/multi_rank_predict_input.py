"""Child program of test_gpu_input_stack_ranks (one process per rank): every rank runs
predict_stack(samples=2, return_std=True, seed=11) on an input-only uint16 stack -- its share of the tiles, two
collectives (one per canvas), every rank pastes -- and checks both canvases, bitwise, against the one-rank result
restated in this process: every tile id, no collective, the same batches of four."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 11


def main():
    from diffsplitting_amd import engine
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
    assert netG.e == 0.01                                          # the sampler's own noise scale: the draws matter
    s = np.random.default_rng(5).integers(0, 6000, (3, 96, 160)).astype(np.uint16)
    nd = dict(mean_input=np.float64(3000.0), std_input=np.float64(1700.0), mean_target=np.array([1500.0, 1500.0]),
              std_target=np.array([850.0, 850.0]), target0_max=None, target1_max=None, input_max=None)
    stack = InputStackTiledPred(s, 64, nd, grid_size=32)
    plan = stack.plan
    assert plan.total == 24 and plan.total % (4 * world) == 0      # every batch is full on every rank

    got, _ = predict_stack(netG, stack, batch_tiles=4, num_timesteps=2, samples=2, return_std=True, seed=SEED)

    means, stds = [], []
    for i in range(0, plan.total, 4):
        chunk = list(range(i, i + 4))
        x = stack.tiles(chunk)["input"]
        mean = m2 = None
        for r in range(2):
            netG.inference(x, continuous=False, num_timesteps=2, seed=SEED, sample_ids=[k + r * plan.total for k in chunk])
            mean, m2 = engine.moments_update(netG.last_full_batch.contiguous(), mean, m2, r)
        m, sd_ = engine.moments_finish(mean, m2, 2)
        means.append(m)
        stds.append(sd_)
    want_mean, want_std = plan.stitch(torch.cat(means)), plan.stitch(torch.cat(stds))

    same_mean = same_bits(got["mean"], want_mean)
    same_std = same_bits(got["std"], want_std)
    spread = bool((got["std"] > 0).any())                          # the two samples do differ: the comparison can fail
    ok = same_mean and same_std and spread
    finish(ok, "PREDICT_INPUT", plan.total, world,
           detail=f"mean equal {same_mean}, std equal {same_std}, spread {spread}")


if __name__ == "__main__":
    main()
