"""The per-launch LPIPS checker of tests/test_gpu_lpips_layers.py (tests/lpips_layer_ref.py), checked on the CPU: it
must accept an honest fp32 evaluation of every launch (torch-CPU float32, its own accumulation order) and reject each of
the small, localised mistakes such a kernel makes -- at the launch the mistake belongs to and at no other.  A mistake
is injected into one stage of the stand-in forward and everything behind it is computed honestly from the wrong stage,
as a device would.  `-m "not gpu"`; run with -s for the ratios."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_layer_ref as L
from tests import lpips_ref as R

torch.set_grad_enabled(False)
LAUNCH = {"x0": "k_lpips_input_nchw", "f1": "k_lpips_conv1", "p1": "k_lpips_pool", "f2": "k_lpips_conv<5>",
          "p2": "k_lpips_pool", "f3": "k_lpips_conv<3>", "f4": "k_lpips_conv<3>", "f5": "k_lpips_conv<3>"}
# 143 x 271: conv1 tiles a 35 x 67 map (3 x 5 tiles), conv2 17 x 33 (2 x 3), conv3..5 8 x 16 (one tile); tap 1 has 37
# partial rows, the last of 41 pixels
H, W, SEED = 143, 271, 11


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def simulate(sd, in0, in1, pre_hook=None, pool_hook=None, finish_hook=None):
    """A forward as the device runs it, every launch in torch-CPU float32 from the previous stage: (table in the layout
    of LPIPS.layer_table(), per_tap (B, 5), total (B,)).  pre_hook = {launch: f(pre, x, w) -> pre} changes a conv's
    result before the ReLU (NCHW), pool_hook = {launch: f(p, x) -> p} a pool's (NCHW), finish_hook f(rows list) ->
    rows list what k_lpips_finish adds."""
    pre_hook, pool_hook = pre_hook or {}, pool_hook or {}
    B = in0.shape[0]
    x = torch.cat([in0, in1]).numpy().astype(np.float32)
    shift, scale = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in (R.SHIFT, R.SCALE))
    h = torch.from_numpy(np.divide(np.subtract(x, shift, dtype=np.float32), scale, dtype=np.float32))
    st = {"x0": h}
    for name in ("conv1", "pool1", "conv2", "pool2", "conv3", "conv4", "conv5"):
        if name in L.CONVS:
            src, dst, l, stride, pad = L.CONVS[name]
            k, idx, _ = R.TRUNK[l]
            w, b = sd[f"net.slice{k}.{idx}.weight"], sd[f"net.slice{k}.{idx}.bias"]
            pre = F.conv2d(st[src], w, b, stride=stride, padding=pad)
            if name in pre_hook:
                pre = pre_hook[name](pre.clone(), st[src], w)
            st[dst] = torch.relu(pre)
        else:
            src, dst = L.POOLS[name]
            p = F.max_pool2d(st[src], 3, 2)
            if name in pool_hook:
                p = pool_hook[name](p.clone(), st[src])
            st[dst] = p
    table = {"pairs": B, "stages": {s: dict(out=_nhwc(t), launch=LAUNCH[s]) for s, t in st.items()}, "taps": []}
    eps = torch.tensor(1e-10, dtype=torch.float32)
    rows_all = []
    for k, s in enumerate(("f1", "f2", "f3", "f4", "f5")):
        f = table["stages"][s]["out"]
        C = f.shape[-1]
        a, c = f[:B].reshape(B, -1, C), f[B:].reshape(B, -1, C)
        w = sd[f"lin{k}.model.1.weight"].reshape(1, 1, C).float()
        q0 = a / ((a * a).sum(-1, keepdim=True).sqrt() + eps)
        q1 = c / ((c * c).sum(-1, keepdim=True).sqrt() + eps)
        d = q0 - q1
        t = w * (d * d)
        assert t.dtype == torch.float32
        hw = a.shape[1]
        rows = L.dist_rows(t.double().sum(-1), hw)
        rows_all.append(rows)
        table["taps"].append(dict(stage=s, launch=f"k_lpips_dist<{C // 64}>", part=rows, nblk=rows.shape[1], hw=hw))
    added = finish_hook(rows_all) if finish_hook else rows_all
    taps64 = torch.stack([r.sum(1) / t["hw"] for r, t in zip(added, table["taps"])], 1)
    return table, taps64.float(), taps64.sum(1).float()


@pytest.fixture(scope="module")
def sd():
    return R.synth_state_dict()


@pytest.fixture(scope="module")
def pair():
    return R.make_pair(1, H, W, SEED)


def bad_launches(sd, pair, **hooks):
    """the launches whose check fails (element bound or aggregate), and the messages"""
    table, per_tap, total = simulate(sd, *pair, **hooks)
    bad, msgs = set(), []
    for name in L.LAUNCHES:
        for v in L.check_launch(name, table, sd, *pair, per_tap, total):
            if not v.ok:
                bad.add(name)
                msgs.append((name, v))
    return bad, msgs


@pytest.mark.parametrize("case", ["pair_143x271", "min_31", "constant_64", "identical_67x71"])
def test_accepts_an_honest_fp32_evaluation(sd, case):
    if case == "pair_143x271":
        in0, in1 = R.make_pair(1, H, W, SEED)
    elif case == "min_31":
        in0, in1 = R.make_pair(2, 31, 31, 12)
    elif case == "constant_64":          # tap-1 features exactly zero: 0 / (0 + 1e-10) in the per-tap check
        in0, in1 = R.constant_image(1, 64, 64), R.make_pair(1, 64, 64, 9)[1]
    else:
        in0 = R.make_pair(1, 67, 71, 13)[0]
        in1 = in0.clone()
    table, per_tap, total = simulate(sd, in0, in1)
    if case == "constant_64":
        assert not table["stages"]["f1"]["out"][:1].any()
    worst, fails = L.check_table(table, sd, in0, in1, per_tap, total)
    print(f"\n{case}: worst error / bound per launch: " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert not fails, fails
    assert set(worst) == set(L.LAUNCHES)
    if case == "pair_143x271":           # the bounds are not slack by orders: the honest error uses a visible part
        assert worst["conv2"] > 0.002 and worst["dist1"] > 0.002, worst


CONV_TILED = ["conv1", "conv2"]          # the levels of this input that have more than one tile


@pytest.mark.parametrize("name", ["conv1", "conv2", "conv3", "conv5"])
def test_rejects_one_dropped_tap_at_a_border_pixel(sd, pair, name):
    _, _, _, stride, pad = L.CONVS[name]

    def drop(pre, x, w):                 # output pixel (0, 3) of image 1 misses tap (pad, pad): input pixel (0, 3 stride)
        pre[1, :, 0, 3] -= w[:, :, pad, pad] @ x[1, :, 0, 3 * stride]
        return pre
    bad, msgs = bad_launches(sd, pair, pre_hook={name: drop})
    assert bad == {name}, msgs
    v = msgs[0][1]
    assert v.index[0] == 1 and v.index[2:] == (0, 3) and name in v.message(), v.message()


@pytest.mark.parametrize("name", CONV_TILED)
def test_rejects_one_tile_shifted_by_one_pixel(sd, pair, name):
    def shift(pre, x, w):                # tile (1, 0): rows 16 .., columns 0 .. 15 hold the values of columns 1 .. 16
        pre[:, :, 16:32, 0:16] = pre[:, :, 16:32, 1:17].clone()
        return pre
    bad, msgs = bad_launches(sd, pair, pre_hook={name: shift})
    assert bad == {name}, msgs
    assert 16 <= msgs[0][1].index[2] < 32 and msgs[0][1].index[3] < 16, msgs[0][1].message()


@pytest.mark.parametrize("name", CONV_TILED)
def test_rejects_a_tile_written_at_the_transposed_grid_position(sd, pair, name):
    """tiles_x and tiles_y mixed up on a non-square grid (3 x 5 and 2 x 3 tiles): the tile computed for grid position
    (0, 1) lands where (1, 0) belongs, as far as the map reaches"""
    def transpose(pre, x, w):
        Hm, Wm = pre.shape[2:]
        assert (Hm + 15) // 16 != (Wm + 15) // 16 and Hm > 16 and Wm > 16
        rows = min(16, Hm - 16)
        pre[:, :, 16:16 + rows, 0:16] = pre[:, :, 0:rows, 16:32].clone()
        return pre
    bad, msgs = bad_launches(sd, pair, pre_hook={name: transpose})
    assert bad == {name}, msgs


@pytest.mark.parametrize("name", ["conv1", "conv2", "conv4"])
def test_rejects_a_halo_filled_with_the_edge_value(sd, pair, name):
    _, _, _, stride, pad = L.CONVS[name]

    def halo(pre, x, w):                 # at one pixel of the last column, image 0
        b = pre[0, :, 2, 0] - F.conv2d(x[:1], w, None, stride=stride, padding=pad)[0, :, 2, 0]          # the bias
        rep = F.conv2d(F.pad(x[:1], (pad,) * 4, mode="replicate"), w, None, stride=stride)
        pre[0, :, 2, -1] = rep[0, :, 2, -1] + b
        return pre
    bad, msgs = bad_launches(sd, pair, pre_hook={name: halo})
    assert bad == {name}, msgs
    Wm = msgs[0][1].index[3]
    assert msgs[0][1].index[0] == 0 and msgs[0][1].index[2] == 2, msgs[0][1].message()
    assert Wm == {"conv1": 66, "conv2": 32, "conv4": 15}[name]


@pytest.mark.parametrize("name", ["pool1", "pool2"])
def test_rejects_one_pool_window_of_2x2(sd, pair, name):
    def small(p, x):
        p[1, :, 3, 2] = x[1, :, 6:8, 4:6].amax(dim=(1, 2))
        return p
    bad, msgs = bad_launches(sd, pair, pool_hook={name: small})
    assert bad == {name}, msgs
    v = msgs[0][1]
    assert v.index[0] == 1 and v.index[2:] == (3, 2) and "k_lpips_pool" in v.message(), v.message()


@pytest.mark.parametrize("name", ["conv1", "conv2", "conv3", "conv4", "conv5"])
def test_rejects_an_output_channel_pair_swapped_inside_a_32_block(sd, pair, name):
    """row_channel(): row 4 of an N block holds channel 16 and row 16 channel 8 -- a packing that takes the row for the
    channel writes channel 4's result where channel 16's belongs (here: in the second 32-channel block)"""
    def swap(pre, x, w):
        pre[:, [36, 48]] = pre[:, [48, 36]]
        return pre
    bad, msgs = bad_launches(sd, pair, pre_hook={name: swap})
    assert bad == {name}, msgs
    assert msgs[0][1].index[1] in (36, 48), msgs[0][1].message()


@pytest.mark.parametrize("tap", [0, 1, 4])
def test_rejects_the_last_partial_row_left_out_of_a_taps_sum(sd, pair, tap):
    def short(rows):
        assert rows[tap].shape[1] > 1 and (rows[tap][:, -1] > 0).all()
        return [r[:, :-1] if k == tap else r for k, r in enumerate(rows)]
    bad, msgs = bad_launches(sd, pair, finish_hook=short)
    assert bad == {"finish"}, msgs
    assert msgs[0][1].index[1] == tap, msgs[0][1].message()


def test_rejects_a_partial_row_that_took_a_pixel_of_its_neighbour(sd, pair):
    """the rows' sum is right, two rows are wrong: what the sum alone would pass"""
    table, per_tap, total = simulate(sd, *pair)
    f = table["stages"]["f1"]["out"]
    v, _, _ = L.dist_reference(f, sd["lin0.model.1.weight"].reshape(-1))
    part = table["taps"][0]["part"].clone()
    part[0, 4] += v[0, 5 * 64]           # the first pixel of row 5 counted in row 4
    part[0, 5] -= v[0, 5 * 64]
    table["taps"][0]["part"] = part
    rows, whole = L.check_launch("dist1", table, sd)
    assert not rows.ok and rows.index in ((0, 4), (0, 5)), rows.message()
    assert whole.ok, whole.message()


def test_reach_tags_from_plain_shapes():
    """tests/test_gpu_lpips_layers.py names what its cases reached with lpips_layer_ref.reach_tags: hand-made shapes
    and their nearest neighbours that must not count"""
    t = L.reach_tags
    assert t({"conv1": (7, 71)}, []) == {"conv1 tiles_x>tiles_y"}
    assert t({"conv2": (35, 3)}, []) == {"conv2 tiles_x<tiles_y"}
    assert t({"conv3": (1, 17)}, []) == {"conv3 tiles_x>tiles_y", "conv3 1mod16"}
    assert t({"conv3": (1, 1)}, []) == {"conv3 1x1"}
    assert t({"conv1": (16, 17)}, []) == {"conv1 0mod16", "conv1 1mod16", "conv1 tiles_x>tiles_y"}
    assert t({"conv1": (15, 18), "conv2": (31, 31)}, []) == {"conv1 tiles_x>tiles_y"}
    assert t({"conv2": (33, 35)}, []) == {"conv2 1mod16"}
    assert t({}, [(1, 65536), (2, 127 * 127)]) == set()
    assert t({}, [(1, 65537)]) == {"dist1 capped"}
    assert L.dist_blocks(66049) == (1024, 65) and L.dist_blocks(65536) == (1024, 64) and L.dist_blocks(9) == (1, 9)
    assert (L.conv1_out(31), L.pool_out(7), L.pool_out(3)) == (7, 3, 1)


def test_geometry_and_the_refusal_before_any_forward(sd):
    """core.lpips.geometry() is the host's stage table restated; layer_table() of a handle that has run nothing is
    refused by the library (no device needed to say so)."""
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.core import lpips as M
    g = M.geometry(271, 287)
    assert [g[s] for s in M.STAGES] == [(271, 287, 3), (67, 71, 64), (33, 35, 64), (33, 35, 192), (16, 17, 192),
                                        (16, 17, 384), (16, 17, 256), (16, 17, 256)]
    assert M.geometry(31, 31)["f5"] == (1, 1, 256) and M.STAGE_LAUNCH == LAUNCH
    table, _, _ = simulate(sd, *R.make_pair(1, 67, 71, 13))
    assert {s: tuple(v["out"].shape[1:]) for s, v in table["stages"].items()} == M.geometry(67, 71)
    with pytest.raises(DsxError, match="H, W >= 31"):
        M.geometry(30, 64)
    fresh = M.LPIPS(state_dict=sd)
    with pytest.raises(DsxError, match="holds no whole forward"):
        fresh.layer_table()
    # the copy takes addresses inside the handle's workspace only: without one, none
    from diffsplitting_amd._lib import lib
    assert lib.dsx_lpips_copy_workspace(fresh._h, 4096, 16, ctypes.c_void_p(256), None) == -1
    assert "not inside the workspace" in lib.dsx_last_error().decode()
