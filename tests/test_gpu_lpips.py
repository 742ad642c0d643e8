"""LPIPS on the MI355X against the float64 restatement (tests/lpips_ref.py).  `-m gpu`.

The tolerance is lpips_ref.bound(): 4 x the error of the same restatement in torch-CPU float32 against float64 over
these very cases, relative, plus a 1e-7 floor -- derived on the CPU, never from the device's output.  Run with -s to see
the measured errors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import nets
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    return R.synth_state_dict()


@pytest.fixture(scope="module")
def model(sd):
    from diffsplitting_amd.core.lpips import LPIPS
    return LPIPS(net='alex', state_dict=sd).cuda()


def _check(name, got, want):
    got, want = got.detach().double().cpu().reshape(want.shape), want.double()
    err, lim = (got - want).abs(), R.bound(want)
    worst = (err / lim).max().item()
    print(f"{name}: max |device - fp64| = {err.max().item():.3e} (relative {(err / want.abs()).max().item():.3e}), "
          f"{worst:.2f} of the bound; yardstick {R.fp32_yardstick():.3e}")
    assert bool((err <= lim).all()), (name, got, want, err, lim)


@pytest.mark.parametrize("case", list(R.CASES))
def test_pairs_match_restatement_total_and_per_tap(model, sd, case):
    in0, in1 = R.make_pair(*R.CASES[case])
    want, want_taps = R.lpips_ref(sd, in0, in1, per_layer=True)
    got, taps = model(in0.cuda(), in1.cuda(), retPerLayer=True)
    assert got.shape == (in0.shape[0], 1, 1, 1) and len(taps) == 5 and taps[0].shape == got.shape
    _check(case, got, want)
    for k in range(5):
        _check(f"{case} tap {k + 1}", taps[k], want_taps[:, k])
    assert torch.equal(model(in0.cuda(), in1.cuda()), got)            # without retPerLayer: the same bits


def test_identical_images_give_exactly_zero(model):
    in0, _ = R.make_pair(3, 97, 131, 4)
    out = model(in0.cuda(), in0.clone().cuda())
    assert torch.equal(out.cpu(), torch.zeros(3, 1, 1, 1))


def test_constant_image_where_the_eps_matters(model, sd):
    in0, in1 = R.constant_image(1, 64, 64), R.make_pair(1, 64, 64, 9)[1]
    want = R.lpips_ref(sd, in0, in1)
    got = model(in0.cuda(), in1.cuda())
    assert torch.isfinite(got).all()
    _check("constant image", got, want)
    assert torch.equal(model(in0.cuda(), in0.cuda()).cpu(), torch.zeros(1, 1, 1, 1))     # 0 / (0 + eps) on both sides


def test_normalize_and_unbatched_input(model):
    in0, in1 = R.make_pair(1, 64, 64, 1)
    a = model(in0.cuda(), in1.cuda())
    assert torch.equal(model((in0.cuda() + 1) / 2 * 2 - 1, (in1.cuda() + 1) / 2 * 2 - 1), model((in0.cuda() + 1) / 2,
                                                                                          (in1.cuda() + 1) / 2,
                                                                                          normalize=True))
    assert torch.equal(model(in0[0].cuda(), in1[0].cuda()), a)        # the notebook passes (3, H, W)
    assert torch.equal(model(in0, in1).cpu(), a.cpu())                # CPU tensors are uploaded


def test_stitched_frames_match_cell_28(model, sd):
    from diffsplitting_amd.core.metrics import calculate_lpips
    tgt, prd = R.make_frames()
    assert tgt.shape == (3, 160, 192, 2)
    want = R.frames_ref(sd, tgt, prd)
    got = calculate_lpips(tgt, prd, model)                            # numpy in, uploaded once
    assert sorted(got) == [0, 1] and all(len(v) == 3 for v in got.values())
    for ch in want:
        _check(f"frames channel {ch}", torch.tensor(got[ch]), want[ch])
    dev = calculate_lpips(torch.from_numpy(tgt).cuda(), torch.from_numpy(prd).cuda(), model)
    assert dev == got
    # the fused input kernel against the plain form on the notebook's own fp32 preparation
    for ch in (0, 1):
        tar, p = R.frames_prepare(tgt, prd, ch)
        plain = model(torch.from_numpy(tar).cuda(), torch.from_numpy(p).cuda()).flatten().tolist()
        assert plain == got[ch]


def test_bitwise_repeatable_and_independent_of_chunking(model):
    in0, in1 = R.make_pair(3, 97, 131, 4)
    a = model(in0.cuda(), in1.cuda(), retPerLayer=True)
    b = model(in0.cuda(), in1.cuda(), retPerLayer=True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    one = model(in0[1:2].cuda(), in1[1:2].cuda())                     # a pair's value does not depend on its batch
    assert torch.equal(one, a[0][1:2])
    tgt, prd = (torch.from_numpy(x).cuda() for x in R.make_frames())
    whole = model.frames(tgt, prd, 0, chunk=3)
    assert torch.equal(model.frames(tgt, prd, 0, chunk=3), whole)
    for chunk in (0, 1, 2):
        assert torch.equal(model.frames(tgt, prd, 0, chunk=chunk), whole), chunk


def test_compat_import_of_lpips(tmp_path, sd):
    """The notebooks' own lines, `import lpips; lpips.LPIPS(net='alex').cuda()`, under the documented PYTHONPATH with
    the weights named by DSX_LPIPS_WEIGHTS."""
    w = tmp_path / "lpips_alex.pth"
    torch.save(sd, w)
    script = tmp_path / "nb.py"
    script.write_text(
        "import sys, torch\n"
        "import lpips\n"
        "loss_fn_vgg = lpips.LPIPS(net='alex').cuda()\n"
        "sys.path.insert(0, %r)\n"
        "from tests import lpips_ref as R\n"
        "a, b = R.make_pair(1, 64, 64, 1)\n"
        "print('compat value %%.9e' %% loss_fn_vgg(torch.Tensor(a[0].numpy()).cuda(), torch.Tensor(b[0].numpy()).cuda()).item())\n"
        % ROOT)
    env = dict(os.environ, DSX_LPIPS_WEIGHTS=str(w),
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "diffsplitting_amd", "compat"), ROOT]))
    r = subprocess.run([sys.executable, str(script)], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "compat value" in r.stdout, r.stderr[-2000:]
    val = float(r.stdout.split("compat value")[1].split()[0])
    a, b = R.make_pair(1, 64, 64, 1)
    want = R.lpips_ref(sd, a, b)
    assert abs(val - want.item()) <= R.bound(want).item()


def test_predict_tiled_returns_lpips_of_its_stitched_output(model):
    from diffsplitting_amd.core.metrics import calculate_lpips
    from diffsplitting_amd.data.tiled_predict import predict_tiled
    from diffsplitting_amd.model import networks
    from tests.util import golden_state_dict
    usd, _ = golden_state_dict("unet_hagen_64")
    netG = networks.define_G(nets.opt(nets.hagen64_section())).cuda()
    netG.load_state_dict({"denoise_fn." + k: v for k, v in usd.items()})
    netG.e = 0.0
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.standard_normal((2, 96, 160)).astype(np.float32)).cuda()
    target = torch.from_numpy(rng.standard_normal((2, 96, 160, 2)).astype(np.float32)).cuda()
    kw = dict(patch_size=64, grid_size=32, batch_tiles=5, sampler_kwargs=dict(num_timesteps=2))
    plain, _ = predict_tiled(netG, frames, **kw)
    (canvas, lp), plan = predict_tiled(netG, frames, lpips=model, target_frames=target, **kw)
    assert torch.equal(canvas, plain)                                 # the option changes nothing else
    assert sorted(lp) == [0, 1] and all(len(v) == 2 and all(np.isfinite(v)) for v in lp.values())
    assert lp == calculate_lpips(target, canvas, model)
    with pytest.raises(ValueError):
        predict_tiled(netG, frames, lpips=model, **kw)
