"""Child program of test_gpu_streams_ranks (one process per rank): every rank predicts its share of the tiles with
per-sample noise streams (seed 11, sample id = tile id) and the sampler's real e = 0.01, one all-gather, every rank
stitches; every rank then checks the result, bitwise, against the one-rank prediction done in this process with the
tile batches taken in REVERSED order -- and that without a seed the two differ, so the comparison can fail."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 11


def main():
    from diffsplitting_amd.data.tiled_predict import predict_tiled
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
    frames = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 96, 160)).astype(np.float32)).cuda()
    kw = dict(patch_size=64, grid_size=32, batch_tiles=4, sampler_kwargs=dict(num_timesteps=2))

    def one_rank_reversed(plan, seed):
        """Every tile id on this rank alone, no collective, the batches of four from the last to the first."""
        outs = {}
        for i in reversed(range(0, plan.total, 4)):
            chunk = list(range(i, min(i + 4, plan.total)))
            extra = {} if seed is None else dict(seed=seed, sample_ids=chunk)
            netG.inference(plan.gather(frames, chunk).unsqueeze(1), continuous=False, num_timesteps=2, **extra)
            outs[i] = netG.last_full_batch.clone()
        return plan.stitch(torch.cat([outs[i] for i in sorted(outs)]))

    pred, plan = predict_tiled(netG, frames, seed=SEED, **kw)
    assert plan.total == 24 and plan.total % (4 * world) == 0      # every batch is full on every rank
    same = same_bits(pred, one_rank_reversed(plan, SEED))
    # without a seed the noise depends on the batching: the same comparison fails
    torch.manual_seed(1)
    plain, _ = predict_tiled(netG, frames, **kw)
    torch.manual_seed(1)
    differs = not torch.equal(plain, one_rank_reversed(plan, None))
    ok = same and differs
    finish(ok, "PREDICT_SEEDED", plan.total, world,
           detail=f"seeded equal {same}, unseeded differs {differs}")


if __name__ == "__main__":
    main()
