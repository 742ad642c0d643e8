"""Per-step frame fusion on the MI355X (`-m gpu`): ``predict_stack(fuse=True)`` with one tile per frame is the unfused
field chain bit for bit; in general it is the test's own restatement (``denoise_fn``, ``engine.solver_step`` and
tests/blend_ref.py on host copies of the tile buffers), whatever the order of the batches, also under the float64 Welford
of two posterior samples; what it is for, measured against the float64 oracle: neighbouring tiles disagree less before the
last blend than the unfused field path leaves them; and ``split --fuse-steps`` end to end."""
import numpy as np
import pytest
import torch

from tests import blend_ref, solver_ref
from tests import tiled_util as T
from tests.bits import same_bits
from tests.tiled_util import SEED, TINY

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SOLVERS = {"ddim0": dict(solver="ddim", steps=4, eta=0.0, spacing=None), "ddim": dict(solver="ddim", steps=4, eta=0.5, spacing=None),
           "dpmpp2m": dict(solver="dpmpp2m", steps=4, eta=0.0, spacing=None)}
BATCH = 4


# ----------------------------------------------------------------------------- 1. one tile per frame: the pinned chain
@pytest.mark.parametrize("name", list(SOLVERS))
def test_one_tile_per_frame_is_the_unfused_chain(name):
    """frames (2, 32, 32), patch 32: gather and blend are copies, so fusion is ``solver_sample_loop`` row by row"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack((2, 32, 32), 32, 16), SOLVERS[name]
    assert stack.plan.total == 2
    kw = dict(batch_tiles=2, solver=solver, seed=SEED, noise="field")
    want, _ = predict_stack(smp, stack, **kw)
    got, _ = predict_stack(smp, stack, fuse=True, **kw)
    assert set(got) == {"mean"} and bool(torch.isfinite(got["mean"]).all()) and same_bits(got["mean"], want["mean"])
    assert same_bits(predict_stack(smp, stack, fuse=True, stitch="blend", window="hann", **kw)[0]["mean"], want["mean"])
    other, _ = predict_stack(smp, stack, fuse=True, **dict(kw, seed=SEED + 1))
    assert not torch.equal(other["mean"], got["mean"])
    assert smp.noise_field is None and smp.noise_source is None


# ----------------------------------------------------------------------------- 2. in general: the restatement
def _restated(smp, stack, solver, batch, id_base=0, window="triangle", reverse=True):
    """The frame state row by row: tiles cut out of the host state with numpy, one UNet forward and one
    engine.solver_step per batch (the batches from the last to the first), noise from the crops of the sample streams,
    the tiles of a row blended on the host by tests/blend_ref.py.  Returns (state (N,H,W,C), the last row's x tiles)."""
    from diffsplitting_amd import engine
    plan = stack.plan
    N, H, W = plan.data_shape
    Cn = 2
    table = smp.solver_table(**solver)
    wy, wx = blend_ref.window_pair(plan, window)
    start = engine.randn_samples((N, Cn, H, W), SEED, [id_base + n for n in range(N)], draw=0)
    X, X0 = np.ascontiguousarray(start.permute(0, 2, 3, 1).cpu().numpy()), None
    starts = list(range(0, plan.total, batch))
    xt = None
    for s in range(table.n_steps):
        xt, x0t = (np.full((plan.total, Cn) + plan.patch_shape[1:], np.nan, dtype=np.float32) for _ in range(2))
        cut, cut0 = blend_ref.cut_tiles(plan, X), None if X0 is None else blend_ref.cut_tiles(plan, X0)
        for i in (reversed(starts) if reverse else starts):
            chunk = list(range(i, min(i + batch, plan.total)))
            B = len(chunk)
            col = lambda name: torch.full((B,), float(getattr(table, name)[s]), device="cuda")
            x = torch.from_numpy(cut[chunk]).cuda()
            net = smp.denoise_fn(torch.cat([stack.tiles(chunk)["input"], x], dim=1), col("tcond").view(B, 1))
            z = T.crops(plan, chunk, Cn, SEED, s + 1, id_base) if table.sigma[s] != 0 else None
            prev = torch.from_numpy(cut0[chunk]).cuda() if table.cp[s] != 0 else None
            x0, xo = engine.solver_step(x, net, col("a"), col("b"), col("cx"), col("c0"), col("sigma"),
                                        cp=None if prev is None else col("cp"), x0_prev=prev, clip=table.clip, z=z)
            xt[chunk], x0t[chunk] = xo.cpu().numpy(), x0.cpu().numpy()
        X = blend_ref.blend_ref(plan, xt, wy, wx)
        if s + 1 < table.n_steps and table.cp[s + 1] != 0:
            X0 = blend_ref.blend_ref(plan, x0t, wy, wx)
    return X, xt


@pytest.mark.parametrize("name", list(SOLVERS))
def test_fusion_is_its_restatement(name):
    """frames (2, 40, 57), patch 32, grid 16: 12 tiles in batches of 4, a shifted last row and column"""
    from diffsplitting_amd.data.tiled_predict import fused_sample, predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS[name]
    plan = stack.plan
    table = smp.solver_table(**solver)
    assert bool(np.any(table.cp != 0)) == (name == "dpmpp2m") and bool(np.any(table.sigma != 0)) == (name == "ddim")
    got, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED, noise="field", fuse=True)
    want, _ = _restated(smp, stack, solver, BATCH)
    assert same_bits(got["mean"].cpu(), torch.from_numpy(want))
    # the driver with its batches in another order, and the other window
    plan.set_window("triangle")
    again = fused_sample(smp, stack, table, BATCH, SEED, 0, order=[2, 0, 1])
    assert same_bits(again, got["mean"])
    hann, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED, noise="field", fuse=True, window="hann")
    assert same_bits(hann["mean"].cpu(), torch.from_numpy(_restated(smp, stack, solver, BATCH, window="hann", reverse=False)[0]))
    assert not torch.equal(hann["mean"], got["mean"])
    unfused, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED, noise="field", stitch="blend")
    assert not torch.equal(unfused["mean"], got["mean"])


def test_a_short_last_batch_is_moved_back():
    """12 tiles in batches of 5: the last batch is tiles 7..11, of which 10 and 11 are kept; one batch size throughout"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS["dpmpp2m"]
    got, _ = predict_stack(smp, stack, batch_tiles=5, solver=solver, seed=SEED, noise="field", fuse=True)
    assert bool(torch.isfinite(got["mean"]).all())
    # every tile of the restatement in a batch of 5 as well: batches 0..4, 5..9 and 7..11, the last keeping two
    want, _ = _restated_batches(smp, stack, solver, [([0, 1, 2, 3, 4], 5), ([5, 6, 7, 8, 9], 5), ([7, 8, 9, 10, 11], 2)])
    assert same_bits(got["mean"].cpu(), torch.from_numpy(want))


def _restated_batches(smp, stack, solver, batches):
    """``_restated`` over explicit (batch, entries kept from its end) pairs; deterministic rows only"""
    from diffsplitting_amd import engine
    plan = stack.plan
    N, H, W = plan.data_shape
    table = smp.solver_table(**solver)
    wy, wx = blend_ref.window_pair(plan, "triangle")
    X = np.ascontiguousarray(engine.randn_samples((N, 2, H, W), SEED, list(range(N)), draw=0).permute(0, 2, 3, 1).cpu().numpy())
    X0, xt = None, None
    for s in range(table.n_steps):
        xt, x0t = (np.full((plan.total, 2) + plan.patch_shape[1:], np.nan, dtype=np.float32) for _ in range(2))
        cut, cut0 = blend_ref.cut_tiles(plan, X), None if X0 is None else blend_ref.cut_tiles(plan, X0)
        for chunk, keep in batches:
            B = len(chunk)
            col = lambda name: torch.full((B,), float(getattr(table, name)[s]), device="cuda")
            x = torch.from_numpy(cut[chunk]).cuda()
            net = smp.denoise_fn(torch.cat([stack.tiles(chunk)["input"], x], dim=1), col("tcond").view(B, 1))
            prev = torch.from_numpy(cut0[chunk]).cuda() if table.cp[s] != 0 else None
            x0, xo = engine.solver_step(x, net, col("a"), col("b"), col("cx"), col("c0"), col("sigma"),
                                        cp=None if prev is None else col("cp"), x0_prev=prev, clip=table.clip)
            xt[chunk[-keep:]], x0t[chunk[-keep:]] = xo.cpu().numpy()[-keep:], x0.cpu().numpy()[-keep:]
        X = blend_ref.blend_ref(plan, xt, wy, wx)
        if s + 1 < table.n_steps and table.cp[s + 1] != 0:
            X0 = blend_ref.blend_ref(plan, x0t, wy, wx)
    return X, xt


def test_fusion_two_samples():
    """sample r takes id_base = r * frames; mean and spread are the float64 Welford of the two restated frame states"""
    from diffsplitting_amd.data.tiled_predict import predict_stack
    smp, stack, solver = T.sr3(), T.stack32(), SOLVERS["ddim"]
    N = stack.plan.data_shape[0]
    got, _ = predict_stack(smp, stack, batch_tiles=BATCH, solver=solver, seed=SEED, noise="field", fuse=True, samples=2,
                           return_std=True)
    xs = [_restated(smp, stack, solver, BATCH, id_base=r * N)[0] for r in range(2)]
    assert not np.array_equal(xs[0], xs[1])
    mean, std = T.welford(xs)
    assert same_bits(got["mean"].cpu(), torch.from_numpy(mean))
    assert same_bits(got["std"].cpu(), torch.from_numpy(std)) and bool((got["std"] > 0).any())


# ----------------------------------------------------------------------------- 3. what it is for
def oracle_seams(plan, table, sd64, cond, start):
    """The float64 oracle (oracle/unet.py under the recurrence of tests/solver_ref.py; deterministic rows, no history) on
    the input tiles ``cond`` (total, 1, p, p) and the frame noise ``start`` (N, C, H, W): the tiles of the last row
    without fusion (every tile diffuses on its own from its crop of the noise) and with it (the tiles are blended in
    float64 after every row and cut out again) -> (tiles_field, tiles_fused)."""
    from oracle import unet as oracle_unet
    cond = np.asarray(cond, dtype=np.float64)
    rows = table.columns()
    assert not np.any(rows["cp"] != 0) and not np.any(rows["sigma"] != 0)

    def net(k, state):
        time = torch.full((state.shape[0], 1), float(table.tcond[k]), dtype=torch.float64)
        inp = torch.from_numpy(np.concatenate([cond, state], axis=1))
        return oracle_unet.unet_forward(sd64, TINY, "sr3", inp, time).numpy()
    X = np.ascontiguousarray(np.asarray(start, dtype=np.float64).transpose(0, 2, 3, 1))
    field = solver_ref.run(rows, blend_ref.cut_tiles(plan, X), net, clip=True, dtype=np.float64)[0][-1]
    wy, wx = blend_ref.window_pair(plan, "triangle")
    fused = None
    for k in range(table.n_steps):
        x = blend_ref.cut_tiles(plan, X)
        _, fused = solver_ref.step({c: rows[c][k] for c in solver_ref.COLUMNS}, x, net(k, x), clip=True, dtype=np.float64)
        X = blend_ref.blend_ref(plan, fused, wy, wx, dtype=np.float64)
    return field, fused


def test_fusion_narrows_what_the_field_leaves():
    """The setting of test_field_noise_narrows_the_seams: ddim, eta = 0, 4 rows, one (1, 64, 96) frame of smooth input,
    all 15 tiles in one batch, the seam RMS over the 12 crop lines -- here of the tiles the LAST ROW produces, before the
    last blend (a blended frame has no crop line): how far neighbouring tiles still disagree.  Without fusion every
    tile diffuses on its own for all rows; with it the neighbours are made equal on their overlap after every row, so
    only the last row's UNet pass (GroupNorm statistics, zero padding at the tile border) separates them.

    The bound on rms_fused / rms_field is twice the ratio of the float64 oracle on the same weights, input and noise,
    and never above 1; the factor 2 is for fp32 and the planner's choice of kernels.  Measured on one MI355X: fused
    0.006394, field 0.320729, ratio 0.019936; the oracle gives the same six digits (largest |device - oracle| over the
    tiles 2.5e-6 fused, 4.2e-6 field), so the bound is 0.0399."""
    from diffsplitting_amd import engine
    from diffsplitting_amd.data.tiled_predict import fused_sample
    smp = T.sr3()
    stack = T.stack((1, 64, 96), 32, 16, seed=2)
    plan = stack.plan
    ids = list(range(plan.total))
    assert plan.total == 15 and all(int(v) % 8 == 0 for v in plan.patch_start[:, 1:].reshape(-1))   # no shifted tile
    solver = SOLVERS["ddim0"]
    table = smp.solver_table(**solver)
    x = stack.tiles(ids)["input"]
    try:
        smp.noise_field = lambda shape, draw: plan.randn_field(ids, shape[1], SEED, draw)
        got = {"field": T.run(smp, x, solver).cpu().numpy()}
    finally:
        smp.noise_field = None
    plan.set_window("triangle")
    rows = []
    fused_sample(smp, stack, table, 15, SEED, 0, keep_tiles=rows)
    assert len(rows) == 4
    got["fused"] = rows[-1].cpu().numpy()
    start = engine.randn_samples((1, 2, 64, 96), SEED, [0], draw=0)
    assert same_bits(plan.gather_canvas(start.permute(0, 2, 3, 1).contiguous()), T.crops(plan, ids, 2, SEED, 0))
    sd64 = {k: v.double() for k, v in smp.weights.items()}
    want = dict(zip(("field", "fused"), oracle_seams(plan, table, sd64, x.cpu().numpy(), start.cpu().numpy())))
    rms = {k: T.seam_rms(plan, got[k])[0] for k in got}
    rms64 = {k: T.seam_rms(plan, want[k])[0] for k in want}
    assert T.seam_rms(plan, got["fused"])[1] == 12
    ratio, ratio64 = rms["fused"] / rms["field"], rms64["fused"] / rms64["field"]
    print(f"\nseam rms over 12 seams before the last blend: fused {rms['fused']:.6f}, field {rms['field']:.6f}, ratio "
          f"{ratio:.6f}; float64 oracle: fused {rms64['fused']:.6f}, field {rms64['field']:.6f}, ratio {ratio64:.6f}")
    print("largest |device - oracle| over the tiles:", {k: float(np.abs(got[k] - want[k]).max()) for k in got})
    assert ratio64 < 1.0
    assert rms["fused"] < rms["field"]
    assert ratio <= min(1.0, 2.0 * ratio64)


# ----------------------------------------------------------------------------- 4. split, end to end
def test_split_fuse_steps_end_to_end(tmp_path):
    """fresh processes at once: --fuse-steps twice (byte for byte the same file), the unfused field run blended and cropped"""
    data = T.split_runs(tmp_path, {"a": ["--fuse-steps"], "b": ["--fuse-steps"], "blend": ["--stitch", "blend"], "crop": []},
                      extra=["--noise-field"])
    assert data["a"] == data["b"] and data["a"] != data["blend"] and data["a"] != data["crop"]
