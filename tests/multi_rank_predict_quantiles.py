"""Child program of test_gpu_quantiles_ranks (one process per rank): every rank runs
predict_stack(samples=3, seed=11, quantiles=(0.1, 0.5, 1.0)) on an input-only uint16 stack -- its share of the tiles, one
collective per canvas, every rank pastes -- and checks the three quantile canvases, bitwise, against the one-rank result
restated in this process: every tile id, no collective, the same batches of four, the draws stacked and sorted by
engine.sample_quantiles (held against the numpy restatement of its contract)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED, SAMPLES, Q = 11, 3, (0.1, 0.5, 1.0)


def main():
    from diffsplitting_amd import engine
    from diffsplitting_amd.data.input_stack import InputStackTiledPred
    from diffsplitting_amd.data.tiled_predict import predict_stack
    from diffsplitting_amd.model import networks
    from tests import nets
    from tests import quantile_ref as REF
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

    got, _ = predict_stack(netG, stack, batch_tiles=4, num_timesteps=2, samples=SAMPLES, seed=SEED, quantiles=Q)

    quants, restated = [], True
    for i in range(0, plan.total, 4):
        chunk = list(range(i, i + 4))
        x = stack.tiles(chunk)["input"]
        draws = []
        for r in range(SAMPLES):
            netG.inference(x, continuous=False, num_timesteps=2, seed=SEED, sample_ids=[k + r * plan.total for k in chunk])
            draws.append(netG.last_full_batch.clone())
        st = torch.stack(draws)
        qt, _ = engine.sample_quantiles(st, Q)
        restated = restated and same_bits(qt.cpu().numpy(), REF.quantiles(st.cpu().numpy(), Q))
        quants.append(qt)
    want = torch.stack([plan.stitch(torch.cat([b[k] for b in quants])) for k in range(len(Q))])

    same = got["quantiles"].shape == want.shape and same_bits(got["quantiles"], want)
    spread = bool((got["quantiles"][0] < got["quantiles"][2]).any())   # the samples do differ: the comparison can fail
    ok = same and restated and spread
    finish(ok, "PREDICT_QUANTILES", plan.total, world,
           detail=f"quantiles equal {same}, kernel equals numpy {restated}, spread {spread}")


if __name__ == "__main__":
    main()
