"""Where a sampling call's normals come from, pinned as a transcript without a GPU: the samplers run on "cpu" against a
recording engine, and every case asserts what was asked of ``noise_source`` / ``engine.randn_samples``, what reached the
engine's loop or ``engine.posterior_step``, and where torch's CPU generator ends -- against an explicit replay of the
expected ``torch.randn`` / ``torch.randint`` calls from the same seed.  Only the public surface is used.

B = 2, 8 x 8; T = 4 for the Gaussian samplers, 3 steps for InDI.  ``noise_field`` needs CUDA tensors and stays with
tests/test_gpu_field.py; here it is only refused."""
import pytest
import torch
from torch import nn

from diffsplitting_amd import engine
from diffsplitting_amd._lib import DsxError
from diffsplitting_amd.model import samplers as S

SEED = 7                    # torch.manual_seed of every run and of its replay
B, HW, T, N = 2, 8, 4, 3
IDS = [5, 9]
SCHED = {"schedule": "linear", "n_timestep": T, "linear_start": 1e-4, "linear_end": 2e-2}
BIT = 1 << 39


def _ints(v):
    return None if v is None else [int(i) for i in v]


def _const(z):
    """What a recorder keeps of injected normals: shape and the first element (the source's call number)."""
    return None if z is None else (tuple(z.shape), float(z.flatten()[0]))


class _Loops:
    """The engine's two loops: record what arrives, leave the state as it is."""

    def __init__(self, log, tag):
        self.log, self.tag = log, tag

    def _record(self, name, table, x, cond=None, noise=None, seed=0, snapshot_steps=(), use_graph=True, stream=None,
                slot=0, sample_ids=None):
        rows = None
        if noise is not None:
            assert noise.dtype == torch.float32
            # the rows that hold a draw, with the first element of every sample's draw
            rows = [(s, noise[s, :, 0, 0, 0].tolist()) for s in range(noise.shape[0]) if bool((noise[s] != 0).any())]
        snaps = [int(s) for s in snapshot_steps]
        self.log.append((self.tag + name, table.n_steps, None if noise is None else tuple(noise.shape), rows, seed,
                         _ints(sample_ids), snaps))
        self.x_init = x.clone()
        return x, (torch.zeros((len(snaps),) + tuple(x.shape)) if snaps else None)

    def sample_loop(self, *a, **k):
        return self._record("sample_loop", *a, **k)

    def solver_loop(self, *a, **k):
        return self._record("solver_loop", *a, **k)


class _Net(nn.Module):
    """A denoise_fn: zeros of the state's shape, and the recording engine."""

    def __init__(self, log, out_channels, tag=""):
        super().__init__()
        self.loops, self.out_channels = _Loops(log, tag), out_channels

    def engine(self):
        return self.loops

    def forward(self, x, time):
        return torch.zeros((x.shape[0], self.out_channels) + tuple(x.shape[2:]))


@pytest.fixture
def log(monkeypatch):
    """The transcript; the engine's device entries are recorders, and a CPU tensor passes for a device one."""
    log = []
    monkeypatch.setattr(S._SamplerBase, "_need_cuda", staticmethod(lambda *a, **k: None))

    def randn_samples(shape, seed, sample_ids, draw=0, device="cuda"):
        log.append(("randn_samples", tuple(shape), seed, _ints(sample_ids), draw))
        return torch.full(tuple(shape), -1.0)

    def posterior_step(x, net, c1, c2, sigma, a=None, b=None, predict_eps=False, clip=False, z=None, seed=0,
                       subsequence=0, repeat_noise=False, x_recon_out=None, mean_out=None, x_out=None, sample_ids=None,
                       draw=None):
        log.append(("posterior_step", _const(z), seed, _ints(sample_ids), draw, bool(repeat_noise)))
        return x_recon_out, mean_out, x_out

    def interp_start(x1, x2, a0, s0, lam, z1=None, z2=None, seed=0, subsequence=0, out=None):
        log.append(("interp_start", _const(z1), _const(z2), seed))
        return torch.zeros_like(x1)

    def q_sample(x0, c0, c2, xe=None, c1=None, z=None, seed=0, subsequence=0, dst=None, coff=0, want_z=False):
        log.append(("q_sample", _const(z), seed))
        return x0, None

    for fn in (randn_samples, posterior_step, interp_start, q_sample):
        monkeypatch.setattr(engine, fn.__name__, fn)
    return log


def _source(log):
    """A ``noise_source`` whose k-th call (from 1) returns the constant k."""
    def source(shape):
        log.append(("source", tuple(shape)))
        return torch.full(shape, float(sum(1 for e in log if e[0] == "source")))
    return source


def _run(call, replay):
    """``call()`` from SEED; torch's generator must end where ``replay()`` from SEED ends.  Returns both results."""
    torch.manual_seed(SEED)
    want = replay()
    end = torch.get_rng_state()
    torch.manual_seed(SEED)
    got = call()
    assert torch.equal(torch.get_rng_state(), end), "torch's CPU generator did not end where the replay ends"
    return got, want


def _randint():
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


def _untouched():
    return None


def _arm(sampler, log, source):
    """Sets the source of a case; returns the seed / sample_ids keywords of its call."""
    if source == "noise_source":
        sampler.noise_source = _source(log)
    return dict(seed=3, sample_ids=IDS) if source == "streams" else {}


SOURCES = ("default", "noise_source", "streams")


# ----------------------------------------------------------------------------- the Gaussian loops
def _gaussian(log, kind, conditional=True):
    cls = S.GaussianSampler if kind == "sr3" else S.GaussianSamplerDdpm
    g = cls(_Net(log, 1), HW, channels=1, conditional=conditional)
    g.set_new_noise_schedule(SCHED, "cpu")
    return g


# method -> (its keywords, the engine loop, rows of the loop, the rows that draw: per kind)
LOOPS = {
    "ancestral": (None, "sample_loop", T, {"sr3": [0, 1, 2], "ddpm": [0, 1, 2, 3]}),
    "ddim0": (dict(steps=3, solver="ddim", eta=0.0), "solver_loop", 3, {"sr3": [], "ddpm": []}),
    "ddim1": (dict(steps=3, solver="ddim", eta=1.0), "solver_loop", 3, {"sr3": [0, 1], "ddpm": [0, 1]}),
    "dpmpp2m": (dict(steps=3, solver="dpmpp2m"), "solver_loop", 3, {"sr3": [], "ddpm": []}),
}


@pytest.mark.parametrize("continous", [False, True])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("method", list(LOOPS))
@pytest.mark.parametrize("kind,conditional", [("sr3", True), ("ddpm", True), ("ddpm", False)])
def test_gaussian_loops(log, kind, conditional, method, source, continous):
    g = _gaussian(log, kind, conditional)
    skw, loop, n, rows = LOOPS[method]
    rows = rows[kind]
    shape = (B, 1, HW, HW)
    x_in = torch.full(shape, 0.5) if conditional else shape
    kw = _arm(g, log, source)
    if skw is None:
        call = lambda: g.p_sample_loop(x_in, continous=continous, **kw)
        snaps = engine.gaussian_snapshot_steps(T) if continous else []
    else:
        call = lambda: g.solver_sample_loop(x_in, continous=continous, **skw, **kw)
        snaps = list(range(n)) if continous else []

    def replay():                                                     # the default source alone touches the generator
        if source != "default":
            return None, None
        x = torch.randn(shape)
        return x, (_randint() if rows else 0)                         # no seed is drawn where no row draws
    out, (x0, seed) = _run(call, replay)

    if source == "default":
        want = [(loop, n, None, None, seed, None, snaps)]
        assert torch.equal(g.denoise_fn.loops.x_init, x0)
    elif source == "noise_source":                                    # call 1: the initial state; then one per drawing row
        noise = [(s, [2.0 + k] * B) for k, s in enumerate(rows)]
        want = [("source", shape)] * (1 + len(rows)) + [(loop, n, ((n,) + shape) if rows else None, noise if rows else None,
                                                         0, None, snaps)]
        assert torch.equal(g.denoise_fn.loops.x_init, torch.ones(shape))
    else:
        want = [("randn_samples", shape, 3, IDS, 0), (loop, n, None, None, 3, IDS, snaps)]
        assert torch.equal(g.denoise_fn.loops.x_init, torch.full(shape, -1.0))
    assert log == want
    assert g.last_full_batch.shape == shape
    if kind == "ddpm" and not conditional:
        assert out is g.last_full_batch                               # the whole batch
    elif continous:                                                   # the start, then the snapshots
        assert out.shape == (B * (1 + len(snaps)), 1, HW, HW)
        assert torch.equal(out[:B], x_in if conditional else x0)
    else:
        assert out.shape == shape[1:] and torch.equal(out, g.last_full_batch[-1])


# ----------------------------------------------------------------------------- InDI
def _indi(log, cls=S.InDISampler):
    i = cls(_Net(log, 2), HW, channels=1, out_channel=2, conditional=False)
    i.set_new_noise_schedule({"n_timestep": N}, "cpu")
    return i


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("t_start", [1.0, [0.5, 0.25]])
def test_indi_inference(log, t_start, source, continuous):
    i = _indi(log)
    x_in = torch.arange(B * HW * HW, dtype=torch.float32).reshape(B, 1, HW, HW) / 64
    xr = torch.cat([x_in] * 2, dim=1)
    shape, one = tuple(xr.shape), (1,) + tuple(xr.shape[1:])
    kw = _arm(i, log, source)
    snaps = engine.indi_snapshot_steps(N) if continuous else []
    out, (d0, seed) = _run(lambda: i.inference(x_in, continuous=continuous, t_float_start=t_start, **kw),
                           lambda: (torch.randn(shape), _randint()) if source == "default" else (None, None))
    per_sample = isinstance(t_start, list)
    if source == "default":
        want = [("sample_loop", N, None, None, seed, None, snaps)]
    elif source == "streams":
        want = [("randn_samples", shape, 3, IDS, 0), ("sample_loop", N, None, None, 3, IDS, snaps)]
        d0 = torch.full(shape, -1.0)
    elif not per_sample:                                              # the start draw, then one per step
        want = [("source", shape)] * (1 + N) + [("sample_loop", N, (N,) + shape, [(s, [2.0 + s] * B) for s in range(N)],
                                                 0, None, snaps)]
        d0 = torch.ones(shape)
    else:                                                             # sample by sample: its start draw, then its steps
        want = [("source", one)] * (B * (1 + N)) + [("sample_loop", N, (N,) + shape,
                                                     [(s, [2.0 + s, 2.0 + s + (1 + N)]) for s in range(N)], 0, None, snaps)]
        d0 = torch.cat([torch.full(one, 1.0), torch.full(one, 2.0 + N)])
    assert log == want
    scale = torch.stack([0.01 * torch.Tensor([t]) for t in (t_start if per_sample else [t_start] * B)]).view(B, 1, 1, 1)
    assert torch.equal(i.denoise_fn.loops.x_init, xr + d0 * scale)
    if continuous:
        assert out.shape == (B * (1 + N), 2, HW, HW) and torch.equal(out[:B], xr + d0 * scale)
    else:
        assert out.shape == one and torch.equal(out, i.last_full_batch[-1:])


@pytest.mark.parametrize("source", SOURCES)
def test_joint_indi_draws_channel_one_first(log, source):
    j = S.JointIndiSampler(None, HW, channels=1, out_channel=1, conditional=False, denoise_fn_ch1=_Net(log, 1, "ch1."),
                           denoise_fn_ch2=_Net(log, 1, "ch2."))
    j.set_new_noise_schedule({"n_timestep": 4}, "cpu")
    j.concurrent = False
    x_in = torch.full((B, 1, HW, HW), 0.5)
    shape = tuple(x_in.shape)
    kw = _arm(j, log, source)
    out, seeds = _run(lambda: j.inference(x_in, num_timesteps=N, **kw),
                      lambda: [(torch.randn(shape), _randint())[1] for _ in range(2)] if source == "default" else None)
    if source == "default":
        want = [("ch1.sample_loop", N, None, None, seeds[0], None, []), ("ch2.sample_loop", N, None, None, seeds[1], None, [])]
    elif source == "noise_source":
        want = []
        for c, tag in enumerate(("ch1.", "ch2.")):
            first = 2.0 + c * (1 + N)
            want += [("source", shape)] * (1 + N) + [(tag + "sample_loop", N, (N,) + shape,
                                                      [(s, [first + s] * B) for s in range(N)], 0, None, [])]
    else:
        ids2 = [v | BIT for v in IDS]
        want = [("randn_samples", shape, 3, IDS, 0), ("ch1.sample_loop", N, None, None, 3, IDS, []),
                ("randn_samples", shape, 3, ids2, 0), ("ch2.sample_loop", N, None, None, 3, ids2, [])]
    assert log == want
    assert out.shape == (1, 2, HW, HW) and j.last_full_batch.shape == (B, 2, HW, HW)
    assert j.indi1.noise_source is j.noise_source and j.indi2.noise_source is j.noise_source
    assert j.indi1.noise_field is None and j.indi2.noise_field is None


# ----------------------------------------------------------------------------- single steps
@pytest.mark.parametrize("source", ["default", "noise_source"])
@pytest.mark.parametrize("kind,t,draws", [("sr3", 2, True), ("sr3", 0, False), ("ddpm", 2, True), ("ddpm", 0, True)])
def test_p_sample(log, kind, t, draws, source):
    """sr3 takes no draw at t == 0; ddpm takes it on every call"""
    g = _gaussian(log, kind, conditional=False)
    x = torch.zeros(B, 1, HW, HW)
    _arm(g, log, source)
    tt = t if kind == "sr3" else torch.full((B,), t, dtype=torch.long)
    _, seed = _run(lambda: g.p_sample(x, tt), lambda: _randint() if draws and source == "default" else 0)
    if draws and source == "noise_source":
        assert log == [("source", tuple(x.shape)), ("posterior_step", (tuple(x.shape), 1.0), 0, None, None, False)]
    else:
        assert log == [("posterior_step", None, seed, None, None, False)]


@pytest.mark.parametrize("source", ["default", "noise_source"])
def test_ddpm_p_sample_repeat_noise(log, source):
    g = _gaussian(log, "ddpm", conditional=False)
    _arm(g, log, source)
    t = torch.full((B,), 2, dtype=torch.long)
    _, seed = _run(lambda: g.p_sample(torch.zeros(B, 1, HW, HW), t, repeat_noise=True),
                   lambda: _randint() if source == "default" else 0)
    one = (1, 1, HW, HW)
    if source == "noise_source":
        assert log == [("source", one), ("posterior_step", (one, 1.0), 0, None, None, True)]
    else:
        assert log == [("posterior_step", None, seed, None, None, True)]


@pytest.mark.parametrize("kind", ["sr3", "ddpm"])
def test_p_sample_seeded_takes_the_loops_draw(log, kind):
    g = _gaussian(log, kind, conditional=False)
    x = torch.zeros(B, 1, HW, HW)
    t = 1 if kind == "sr3" else torch.full((B,), 1, dtype=torch.long)
    _run(lambda: g.p_sample_seeded(x, t, 3, IDS), _untouched)
    _run(lambda: g.p_sample_seeded(x, t, 3, IDS, draw=9), _untouched)
    assert log == [("posterior_step", None, 3, IDS, T - 1, False), ("posterior_step", None, 3, IDS, 9, False)]
    with pytest.raises(DsxError, match="p_sample_seeded needs sample_ids"):
        g.p_sample_seeded(x, t, None, None)
    with pytest.raises(DsxError, match="only together with sample_ids"):
        g.p_sample_seeded(x, t, 3, None)


@pytest.mark.parametrize("source", SOURCES)
def test_indi_one_step(log, source):
    i = _indi(log)
    x = torch.zeros(B, 2, HW, HW)
    _arm(i, log, source)
    if source == "streams":
        _run(lambda: i.inference_one_step_seeded(x, 0.25, 0.5, 3, IDS, 2), _untouched)
        assert log == [("posterior_step", None, 3, IDS, 2, False)]
        with pytest.raises(DsxError, match="inference_one_step_seeded needs sample_ids"):
            i.inference_one_step_seeded(x, 0.25, 0.5, None, None, 2)
        return
    _, seed = _run(lambda: i.inference_one_step(x, 0.25, 0.5), lambda: _randint() if source == "default" else 0)
    if source == "noise_source":
        assert log == [("source", tuple(x.shape)), ("posterior_step", (tuple(x.shape), 1.0), 0, None, None, False)]
    else:
        assert log == [("posterior_step", None, seed, None, None, False)]


@pytest.mark.parametrize("source", ["default", "noise_source"])
@pytest.mark.parametrize("t", [0, 2])
def test_ddpm_interpolate(log, t, source):
    """x1's draw, x2's, then one per step; by default a seed for the start and one for the loop.  ``noise_field`` is
    not consulted."""
    g = _gaussian(log, "ddpm", conditional=False)
    _arm(g, log, source)
    g.noise_field = lambda *a: pytest.fail("interpolate asked the noise field")
    x1, x2 = torch.zeros(B, 1, HW, HW), torch.ones(B, 1, HW, HW)
    shape = tuple(x1.shape)
    out, seeds = _run(lambda: g.interpolate(x1, x2, t=t),
                      lambda: [_randint() for _ in range(2 if t else 1)] if source == "default" else None)
    if source == "default":
        want = [("interp_start", None, None, seeds[0])] + ([("sample_loop", t, None, None, seeds[1], None, [])] if t else [])
    else:
        want = [("source", shape)] * 2 + [("interp_start", (shape, 1.0), (shape, 2.0), 0)]
        if t:
            want += [("source", shape)] * t + [("sample_loop", t, (t,) + shape, [(s, [3.0 + s] * B) for s in range(t)],
                                                0, None, [])]
    assert log == want and out.shape == shape


@pytest.mark.parametrize("source", ["default", "noise_source", "given"])
def test_ddpm_q_sample(log, source):
    g = _gaussian(log, "ddpm", conditional=False)
    _arm(g, log, source)
    x = torch.zeros(B, 1, HW, HW)
    noise = torch.full(tuple(x.shape), 4.0) if source == "given" else None
    _, seed = _run(lambda: g.q_sample(x, torch.full((B,), 2, dtype=torch.long), noise=noise),
                   lambda: _randint() if source == "default" else 0)
    if source == "default":
        assert log == [("q_sample", None, seed)]
    elif source == "given":
        assert log == [("q_sample", (tuple(x.shape), 4.0), 0)]
    else:
        assert log == [("source", tuple(x.shape)), ("q_sample", (tuple(x.shape), 1.0), 0)]


# ----------------------------------------------------------------------------- refusals leave everything alone
def test_a_refused_call_draws_nothing(log):
    g, i = _gaussian(log, "sr3"), _indi(log)
    x = torch.zeros(B, 1, HW, HW)
    for s in (g, i):
        s.noise_field = lambda *a: pytest.fail("the noise field was asked before the refusal")
    calls = [lambda **kw: g.p_sample_loop(x, **kw), lambda **kw: g.solver_sample_loop(x, steps=3, **kw),
             lambda **kw: i.inference(x, **kw), lambda **kw: i.inference(x, t_float_start=[0.5, 0.25], **kw)]
    torch.manual_seed(SEED)
    state = torch.get_rng_state()
    for call in calls:
        with pytest.raises(DsxError, match="noise_field together with sample_ids"):
            call(seed=3, sample_ids=IDS)
        with pytest.raises(DsxError, match="only together with sample_ids"):     # the field checks come first
            call(seed=3)
    for s in (g, i):
        s.noise_field = None
    for call in calls:
        with pytest.raises(DsxError, match="sample_ids need seed"):
            call(sample_ids=IDS)
        with pytest.raises(DsxError, match="B = 2 ids"):
            call(seed=3, sample_ids=[1, 2, 3])
    for s in (g, i):
        s.noise_source = _source(log)
    for call in calls:
        with pytest.raises(DsxError, match="noise_source together with sample_ids"):
            call(seed=3, sample_ids=IDS)
    assert log == [] and torch.equal(torch.get_rng_state(), state)
