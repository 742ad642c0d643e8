"""One UNet forward with every conv, attention, GroupNorm-statistics, FiLM and input-staging launch checked against a
float64 reference of that one layer (tests/layer_ref.py: the references and their bounds), computed from the tensors
the launch actually read (the executor's layer table: the workspace is never reused, so after a forward every
intermediate is still there).  Shared by tests/test_gpu_layers.py (the golden models), tests/test_gpu_widths.py
(models at other channel widths) and tests/test_gpu_groups.py (GroupNorm groups wider than 64 channels): the caller
names the case and brings the state dict."""
import math
import re

import torch

from tests import layer_ref
from tests.gpu_util import build_engine

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

# every variant tag a checked launch may carry; a new kernel variant must be added here (and so get checked)
# (the tiles are ConvTile of dsx_kernels.h)
KNOWN_TAGS = {"first", "img", "g2", "ws", "ws c2", "ws c4", "+gn", "splitK", "s2", "up", "naive", "attn", "stage1",
              "stage2",
              "tile256x128", "tile128x128", "tile64x128", "tile256x64", "tile128x64", "tile64x64", "tile128x32",
              "tile256x32"}
# (stage1 / stage2: staging modes of k_conv_mfma / k_conv_ws, derived from the layer's shapes, see stage_tag.)

# the plain fields of a layer-table entry that check_plan hands back (no tensors: what a caller derives reach tags from)
LAYER_FIELDS = ("kind", "ks", "stride", "up", "swish", "B", "Hs", "Ws", "Ho", "Wo", "C0", "C1", "Cout", "gn_in_kernel",
                "bias_in_film", "resid_ld", "out_ld", "desc", "w_name")


def stage_tag(L, dt):
    """k_conv_mfma / k_conv_ws staging mode of a conv (plan_conv): 1 = a concat whose first source ends inside a staged
    group, 2 = a source that is not a whole number of 16-byte units"""
    if {"first", "img", "naive"} & launch_tags(L["desc"]):
        return set()
    um, kc = (3, 16) if dt == "f32" else (7, 32)
    gw = (2 if L["ks"] == 1 else 1) * kc
    C0, C1 = L["C0"], L["C1"]
    mode = 2 if (C0 & um or C1 & um) else (0 if (C1 == 0 or C0 % gw == 0) else 1)
    return {f"stage{mode}"} if mode else set()


def launch_tags(desc):
    tok = desc.split()
    if not tok:
        return set()
    tags = set()
    head = tok[0]
    if head == "attn":
        return {"attn"}
    if head.endswith("-naive"):
        tags.add("naive")
    if head.endswith("s2"):
        tags.add("s2")
    if head.endswith("up"):
        tags.add("up")
    for i, t in enumerate(tok[1:], 1):
        if t in ("first", "img", "g2", "+gn"):
            tags.add(t)
        elif t == "ws":
            tags.add("ws")
            if i + 1 < len(tok) and tok[i + 1] in ("c2", "c4"):
                tags.add("ws " + tok[i + 1])
        elif t.startswith("splitK"):
            tags.add("splitK")
        elif t.startswith("tile"):
            tags.add(t)
    return tags


def reach_tags(L, dt, groups):
    """the reach conditions of tests/test_gpu_widths.py that one layer-table entry meets (its plain fields, as check_plan
    hands them back): kernel paths that only channel counts off 16 2^k take"""
    if L["kind"] == 1:                                   # attention at a head dimension that is no power of two
        return {"attn"} if L["C0"] & (L["C0"] - 1) else set()
    if L["kind"] != 0:
        return set()
    out = set()
    tags = launch_tags(L["desc"])
    cin, cout = L["C0"] + L["C1"], L["Cout"]
    if L["gn_scale"] or L["gn_in_kernel"]:
        cpg = cin // groups
        if cpg == 3:
            out.add("cpg3")
        if cpg >= 5 and cpg & (cpg - 1):
            out.add("cpg5+")
    if {"first", "img", "naive"} & tags:
        return out
    if cout % 16:                                        # the scalar epilogue (k_conv_mfma: vec == false)
        if L["resid"]:
            out.add("scalar+resid")
        if L["film"]:
            out.add("scalar+film")
        if cout > 16:
            out.add("scalar nbase>0")
    if "stage2" in stage_tag(L, dt):
        for cond, t in ((L["gn_scale"], "stage2+gn"), (L["C1"] > 0, "stage2+cat"), (L["ks"] == 1, "stage2 1x1"),
                        (L["stride"] == 2, "stage2 s2"), (L["up"], "stage2 up")):
            if cond:
                out.add(t)
    m = re.search(r"splitK(\d+)", L["desc"])
    if m and int(m.group(1)) & (int(m.group(1)) - 1):
        out.add("splitK odd")
    if "ws" in tags:                                     # channels per staged group of k_conv_ws (decide_ws_chunks)
        chunks = 4 if "ws c4" in tags else (2 if ("ws c2" in tags or L["ks"] == 1) else 1)
        if cin % (chunks * (16 if dt == "f32" else 32)):
            out.add("ws ktail")
    m = re.search(r"tile\d+x(\d+)", L["desc"])
    if m and int(m.group(1)) >= 128 and cout % int(m.group(1)):
        out.add("wide ntail")
    return out


def finalizes(ops, groups):
    """The GroupNorm finalizes of a plan, from its launches (tests/plan_dump.py read_dump of a DSX_PLAN_DUMP file):
    [dict(host, cpg, C0, C1, nchunk0, nchunk1, f32, shifted, consumer)], `host` the kernel that runs gn_finalize_item --
    "gn_finalize" / "gn_finalize_wide" for a launch of its own (the dump names the launcher by the launch rule), "hosted"
    for the finalize that the residual 1 x 1 k_conv_ws launch in front of the consumer runs (a `+gn` launch; that
    GroupNorm has one source, the block's first conv, whose epilogue left fp32 partials: plan_res hosts nothing else).
    `f32` / `shifted`: a source's partials are fp32 / carry a pivot.  `consumer`: the conv launch that reads the scale
    and shift.  The layer table does not say which kernel finalized a GroupNorm; the dump does."""
    from tests.plan_dump import FIN_LAUNCHERS
    out = []
    for i, op in enumerate(ops):
        c = op["conv"]
        if op["launcher"] in FIN_LAUNCHERS:
            f = op["fin"]
            assert f.groups == groups and ops[i + 1]["conv"] is not None and ops[i + 1]["conv"].has_gn, op["desc"]
            out.append(dict(host=op["launcher"], cpg=(f.C0 + f.C1) // groups, C0=f.C0, C1=f.C1, nchunk0=f.nchunk0,
                            nchunk1=f.nchunk1, f32=bool(f.f32_0 or (f.C1 and f.f32_1)),
                            shifted=any(p.bias or p.film for p in (f.piv0, f.piv1)), consumer=ops[i + 1]))
        elif c is not None and c.has_gn and op["launcher"] in ("conv_mfma", "conv_ws"):
            prev = ops[i - 1]
            if prev["launcher"] in FIN_LAUNCHERS:
                continue
            # no finalize launch in front (split-K: the main launch is in front of its reduce, which is not a conv)
            assert prev["launcher"] == "conv_ws" and prev["desc"].endswith(" +gn") and prev["ks"] == 1, \
                (prev["desc"], op["desc"])
            assert c.C1 == 0, op["desc"]
            out.append(dict(host="hosted", cpg=c.C0 // groups, C0=c.C0, C1=0, nchunk0=None, nchunk1=0, f32=True,
                            shifted=None, consumer=op))
    return out


def group_reach_tags(ops, groups):
    """the reach conditions of tests/test_gpu_groups.py that the launches `ops` of one plan meet: GroupNorm groups wider
    than 64 channels in each of the three hosts of gn_finalize_item, and the 8 x 8 convs k_conv_img turns away"""
    out = set()
    for f in finalizes(ops, groups):
        cpg = f["cpg"]
        if cpg <= 64:
            continue
        if f["host"] == "gn_finalize":
            out.add("fin>64")                  # one wave: the tail loop of gn_finalize_item
        elif f["host"] == "gn_finalize_wide":
            out.add("wide own>64" if cpg <= 256 else "wide>256")      # waves 1 .. 3 own channels / the tail loop
        else:
            out.add("hosted>64")
        if f["C1"] and f["C0"] % cpg:
            out.add("straddle>64")
        if f["f32"]:
            out.add("f32part>64")
        if f["shifted"]:                       # (a launch of its own whose fp32 partials carry a pivot)
            out.add("shifted>64")
        if cpg & (cpg - 1):
            out.add("npow2>64")
    for op in ops:
        c = op["conv"]
        if (c is not None and c.has_gn and op["launcher"] != "conv_img"
                and (c.Hs, c.Ws, c.Ho, c.Wo) == (8, 8, 8, 8)):
            out.add("8x8 no img")
    return out


def pow2_divisor(v, cap):
    """largest power of two that divides v and is <= cap (dsx_plan.cpp)"""
    p = 1
    while p * 2 <= cap and v % (p * 2) == 0:
        p *= 2
    return p


def geom_tag(L):
    """The geometry class of a conv launch of the MFMA families, e.g. "ws 3x3 4x16x1@64" or "mfma 3x3 s2 8x4x2@64+tail":
    family (mfma, g2, splitK, ws), kernel size with s2 / up, the tile TW x TH x TB in output pixels and images, the
    tile's pixel count BM, and +tail when the last tile of a launch misses images (B % TB != 0).  None for every other
    launch (attention, first / img / naive convs).  The tile is not in the layer table: it is derived from the output map
    by the planner's rule (tile_geometry in dsx_plan.cpp): TW = the largest power of two <= 16 dividing Wo, TH = the
    largest <= BM / TW dividing Ho, TB = BM / (TW TH).  tests/test_planner_cpu.py holds this against the tile the planner
    wrote into each launch's arguments."""
    if L["kind"] != 0:
        return None
    tags = launch_tags(L["desc"])
    m = re.search(r"\btile(\d+)x\d+\b", L["desc"])
    if {"first", "img", "naive"} & tags or not m:
        return None
    BM = int(m.group(1))
    TW = pow2_divisor(L["Wo"], 16)
    TH = pow2_divisor(L["Ho"], max(1, BM // TW))
    TB = BM // (TW * TH)
    assert TB >= 1 and TW * TH * TB == BM, (L["desc"], TW, TH, BM)      # the planner admits nothing else
    fam = "splitK" if "splitK" in tags else ("ws" if "ws" in tags else ("g2" if "g2" in tags else "mfma"))
    size = f"{L['ks']}x{L['ks']}" + (" s2" if L["stride"] == 2 else "") + (" up" if L["up"] else "")
    return f"{fam} {size} {TW}x{TH}x{TB}@{BM}" + ("+tail" if L["B"] % TB else "")


def inputs(case, B, H, W, flat=False, ddpm_t=None):
    """seeded (x, t) of one forward; `ddpm_t`: the time tensor of a ddpm-flavour case ((1,) or (B,) values)"""
    g = torch.Generator().manual_seed(1000 + B * 7 + H + W)
    cin = case["cfg"]["in_channel"]
    x = (1e-4 if flat else 1.0) * torch.randn((B, cin, H, W), generator=g)
    if case["flavour"] == "sr3":
        t = 0.05 + 0.95 * torch.rand((B, 1), generator=g)
    else:
        t = ddpm_t
    return x, t


def film_reference(sd, case, t, B):
    """fp64 time MLP (sr3 PositionalEncoding / ddpm TimeEmbedding) and the stacked per-block linears, with an
    absolute error bound propagated through every fp32 step the kernel takes (each <= u32 relative, accumulations at
    4 sqrt(K) u32, sin/cos arguments rounded to fp32: <= 2 u32 (1 + |arg|))"""
    U = layer_ref.U32
    sd = {k: v.to(torch.float64) for k, v in sd.items()}
    inner = case["cfg"]["inner_channel"]
    tt = t.reshape(-1).to(torch.float64)
    if tt.numel() == 1:
        tt = tt.expand(B)
    if case["flavour"] == "sr3":
        freq = torch.exp(-math.log(1e4) * torch.arange(inner // 2, dtype=torch.float64) / (inner // 2))
        p1, p3 = "noise_level_mlp.1", "noise_level_mlp.3"
    else:
        freq = sd["time_mlp.0.inv_freq"]
        p1, p3 = "time_mlp.1", "time_mlp.3"
    arg = tt[:, None] * freq[None, :]
    enc = torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)
    e = 2 * U * (1 + torch.cat([arg, arg], dim=-1).abs())

    def lin(h, eh, w, b):
        K = w.shape[1]
        y = h @ w.T + b
        S = h.abs() @ w.abs().T + b.abs()
        return y, eh @ w.abs().T + 4 * math.sqrt(K + 1) * U * S

    def sw(h, eh):
        a = layer_ref.swish(h)
        return a, 1.1 * eh + 4 * U * a.abs()
    h, eh = sw(*lin(enc, e, sd[p1 + ".weight"], sd[p1 + ".bias"]))
    h, eh = lin(h, eh, sd[p3 + ".weight"], sd[p3 + ".bias"])
    if case["flavour"] != "sr3":
        h, eh = sw(h, eh)
    return h, eh, sd


def check_plan(plan, case, sd, dt, B, H, W, env, x, t, dev, monkeypatch, flat=False):
    """Builds the engine of `case` (a dict with `cfg` and `flavour`) from the state dict `sd` in operand type `dt` under
    the planner knobs `env`, runs one forward of (x, t) and checks every layer.  Asserts that no check failed and that
    no launch carries a tag outside KNOWN_TAGS; returns dict(dtype, tags, layers, worst, table, y): `table` the plain
    fields of every layer (LAYER_FIELDS, plus whether it has a residual / FiLM vector / finalized GroupNorm), `y` the
    forward's output.  A conv entry of `table` with a finalized GroupNorm also has `gn_ratio`, the largest |mean| / std
    of its groups (None elsewhere)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    groups = case["cfg"]["norm_groups"]
    op = DT[dt]
    eng = build_engine(case["cfg"], case["flavour"], sd, dtype=dt)
    y = eng.forward(x.to(dev), t.to(dev))
    table = eng.layer_table(B, H, W)
    assert eng.handoff_timeouts() == 0
    images = [0, B - 1] if B >= 4 else None
    fails, tags, worst, n = [], set(), (0.0, ""), 0
    max_gn_ratio = 0.0
    gn_ratio = {}                                      # layer index -> largest |mean| / std of a group
    film_h, film_e, sd64 = film_reference(sd, case, t, B)
    film_h, film_e = film_h.to(dev), film_e.to(dev)

    def note(v, what):
        nonlocal worst
        if v.ratio > worst[0]:
            worst = (v.ratio, what)
        if not v.ok:
            fails.append(v.message())

    for li, L in enumerate(table):
        kind = L["kind"]
        if kind == 3:                                  # staged input: bit-equal to round_T(x) in NHWC
            ref = x[:, L["C0"]:L["C0"] + L["Cout"]].permute(0, 2, 3, 1).to(dev).to(L["out"].dtype)
            if not torch.equal(L["out"], ref):
                fails.append(f"input staging (channels {L['C0']}..): not bit-equal to round_T(x)")
            n += 1
            continue
        if kind == 2:                                  # FiLM vector: checked below, per block
            continue
        n += 1
        tags |= launch_tags(L["desc"])
        where = f"[{plan}] {L['desc']} ({L['w_name'] or 'attention'})"
        if kind == 1:
            note(layer_ref.check_attention(L, op, images, where), where)
            continue
        tags |= stage_tag(L, dt)
        w = sd[L["w_name"]].to(dev)
        bias = None if (L["bias_in_film"] or L["b_name"] is None) else sd[L["b_name"]].to(dev)
        gamma = sd[L["gn_gamma_name"]].to(dev) if L["gn_gamma_name"] else None
        beta = sd[L["gn_beta_name"]].to(dev) if L["gn_beta_name"] else None
        # k_conv_naive multiplies fp32 weights by the fp32 activation in every build: its operands are not rounded
        op_conv = torch.float32 if "naive" in launch_tags(L["desc"]) else op
        note(layer_ref.check_conv(L, w, bias, gamma, beta, groups, op_conv, images, where), where)
        if L["gn_scale"] is not None:
            v1, v2, r = layer_ref.check_gn_stats(L, gamma, beta, groups, op, where)
            max_gn_ratio = max(max_gn_ratio, r)
            gn_ratio[li] = r
            note(v1, where + " gn_scale")
            note(v2, where + " gn_shift")
        if L["film"] is not None:
            rb = L["w_name"][:-len(".block1.block.3.weight")]
            lk = rb + (".noise_func.noise_func.0" if case["flavour"] == "sr3" else ".mlp.1")
            wf, bf = sd64[lk + ".weight"].to(dev), sd64[lk + ".bias"].to(dev)
            ref = film_h @ wf.T + bf
            S = film_h.abs() @ wf.abs().T + bf.abs()
            if L["bias_in_film"]:
                cb = sd64[L["b_name"]].to(dev)
                ref, S = ref + cb, S + cb.abs()
            bound = film_e @ wf.abs().T + 4 * math.sqrt(wf.shape[1] + 2) * layer_ref.U32 * S
            fv = layer_ref.Verdict(L["film"].to(torch.float64), ref, bound, torch.zeros_like(ref), where + " film")
            fv.aggregate = []
            note(fv, where + " film")
    assert eng.handoff_timeouts() == 0
    print(f"\n{plan}: {n} layers checked, worst error/bound {worst[0]:.3f} at {worst[1]}; "
          f"max |mean|/std of a GroupNorm group {max_gn_ratio:.3g}")
    if flat:
        assert max_gn_ratio > 1e3, f"the flat case should reach |mean|/std > 1e3, got {max_gn_ratio:.3g}"
    assert not fails, f"{len(fails)} check(s) failed:\n" + "\n".join(fails[:20])
    unknown = tags - KNOWN_TAGS
    assert not unknown, f"launch variants without per-layer coverage: {unknown}"
    light = []
    for li, L in enumerate(table):
        d = {k: L[k] for k in LAYER_FIELDS}
        d["gn_ratio"] = gn_ratio.get(li)
        for k in ("resid", "film", "gn_scale"):          # (only a conv's entries hold tensors under these names)
            d[k] = L["kind"] == 0 and L[k] is not None
        light.append(d)
    return dict(dtype=dt, tags=tags, layers=n, worst=worst, table=light, y=y)
