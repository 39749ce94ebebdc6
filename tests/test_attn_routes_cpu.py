"""The routing table of fk_attn_fwd / fk_attn_bwd, pinned through the host-side query (kernels.attn_route: no launch, no GPU), and the
conditions under which the inputs of tests/attn_inputs.py make tests/test_attn_routes_gpu.py worth running: on the float64 reference
alone, for every case of tests/cases.py's ATTN_ROUTE_CASES,
  * a CPU model of the kernels' documented roundings stays inside the bound (so the bound does not fail a correct kernel);
  * hiding any visible cell of 64 query rows x 64 keys moves o and dq by at least 2x the bound somewhere in those rows and dk and dv by
    at least 2x the bound somewhere in those keys (rows the cell would leave empty keep it);
  * moving the visible edge of any row by one key, either way, moves o by at least 2x the bound in that row.
2x: a real kernel's own error is at most 1x the bound and may oppose the defect; at 2x the defect still fails the GPU test."""
import functools
import re
from pathlib import Path

import pytest
import torch

from tests import attn_inputs as AI
from tests import cases

BF, F32 = torch.bfloat16, torch.float32
ALL = cases.ATTN_ROUTE_CASES + cases.ATTN_SPIKE_CASES
T = AI.TILE


@pytest.fixture(scope="module")
def K():
    from frankenstein_amd import build
    build.build(verbose=False)
    from frankenstein_amd import kernels
    return kernels


def cid(c):
    return c["id"]


def case_routes(K, c):
    vis, extras = AI.visibility(c)
    return K.attn_route_names(c["Nq"], c["Nk"], c["D"], BF if c["dtype"] == "bf16" else F32, AI.make_mask(K, c, extras, vis, "cpu"), q_prescaled=c["ps"])


# ----------------------------------------------------------------------------------------------- routes
def test_route_constants_match_the_header(K):
    hdr = (Path(__file__).resolve().parents[1] / "include" / "franken_hip.h").read_text()
    for first, names in (("FK_ATTN_FWD_GENERIC", K.ATTN_FWD_ROUTE_NAMES), ("FK_ATTN_DQ_GENERIC", K.ATTN_DQ_ROUTE_NAMES), ("FK_ATTN_DKDV_GENERIC", K.ATTN_DKDV_ROUTE_NAMES)):
        enum = re.search(r"enum \{ (" + first + r"[^}]*) \};", hdr).group(1)
        vals = {k.strip()[len("FK_ATTN_"):]: int(v) for k, v in (e.split("=") for e in enum.split(","))}
        assert vals == {n: v for v, n in names.items()} and sorted(vals.values()) == list(range(4))


@pytest.mark.parametrize("case", ALL, ids=cid)
def test_cases_reach_the_routes_they_name(K, case):
    assert case_routes(K, case) == case["routes"]
    assert case["Nk"] <= 1152 and case["B"] <= 3 and case["H"] <= 3


def _where(pred):
    return [c for c in cases.ATTN_ROUTE_CASES if pred(c)]


def test_the_matrix_covers_every_route_and_every_phase():
    C = cases.ATTN_ROUTE_CASES
    assert {c["routes"][0] for c in C} == {"FWD_GENERIC", "FWD_FEWQ", "FWD_PS", "FWD_ASM"}
    assert {c["routes"][1] for c in C} == {"DQ_GENERIC", "DQ_FEWQ", "DQ_PS", "DQ_ASM"}
    assert {c["routes"][2] for c in C} == {"DKDV_GENERIC", "DKDV_PS", "DKDV_ASM", "DKDVW_ASM"}
    for i, routes in enumerate((("FWD_GENERIC", "FWD_FEWQ", "FWD_PS", "FWD_ASM"), ("DQ_GENERIC", "DQ_FEWQ", "DQ_PS", "DQ_ASM"),
                                ("DKDV_GENERIC", "DKDV_PS", "DKDV_ASM", "DKDVW_ASM"))):
        for r in routes:                                      # every route with more than one sample and more than one head
            assert any(c["B"] > 1 and c["H"] > 1 for c in C if c["routes"][i] == r), r
    plain = lambda c: c["mask"] == ("none",)
    # the forward stream: 2 .. 9 key tiles (warm-up, first / steady / drain steps at every phase of the ring of 4)
    assert {c["Nk"] // 64 for c in _where(lambda c: c["routes"][0] == "FWD_ASM" and plain(c))} >= set(range(2, 10))
    # the wide dK/dV stream: 1, 2, 3, 4, 7 query tiles (slots 0, 1, 2 of the ring of 3 and the wrap)
    assert {c["Nq"] // 64 for c in _where(lambda c: c["routes"][2] == "DKDVW_ASM" and plain(c))} >= {1, 2, 3, 4, 7}
    assert {c["Nq"] // 64 for c in _where(lambda c: c["routes"][2] == "DKDV_ASM" and plain(c))} >= {1, 2, 5}
    assert {c["Nk"] // 64 for c in _where(lambda c: c["routes"][1] == "DQ_ASM" and plain(c))} >= {1, 2, 5}
    # the pre-scaled tile loops: ragged, causal, block-causal 8 and 128, sliced offsets, prefix and key-padding tables
    ps = _where(lambda c: c["routes"] == ("FWD_PS", "DQ_PS", "DKDV_PS"))
    assert {c["mask"][0] for c in ps} >= {"none", "causal", "block", "sliced", "prefix", "keypad"}
    assert {c["mask"][1] for c in ps if c["mask"][0] == "block"} >= {8, 128}
    assert any(c["Nq"] % 64 and c["Nk"] % 64 for c in ps)
    # few queries: Nq 8 and 32, Nk 1024 and a ragged value above it
    fq = _where(lambda c: c["routes"][0] == "FWD_FEWQ" and c["routes"][1] == "DQ_FEWQ")
    assert {c["Nq"] for c in fq} == {8, 32} and 1024 in {c["Nk"] for c in fq} and any(c["Nk"] > 1024 and c["Nk"] % 64 for c in fq)
    # the generic kernels: fp32 D 8 / 16 / 32 / 64, bf16 D 8 / 16 / 32 / 128, every mask kind, dense with per-head tables
    gen = _where(lambda c: c["routes"] == ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC"))
    assert {c["D"] for c in gen if c["dtype"] == "f32"} == {8, 16, 32, 64} and {c["D"] for c in gen if c["dtype"] == "bf16"} >= {8, 16, 32, 128}
    assert {c["mask"][0] for c in gen} == {"none", "causal", "block", "sliced", "prefix", "keypad", "dense"}
    assert any(c["mask"][0] == "dense" and c["mask"][2] == c["H"] > 1 for c in gen) and any(c["mask"][0] == "dense" and c["mask"][1:] == (1, 1) for c in gen)
    # the spike cases: a late spike and an all-negative head on both pre-scaled forward kernels
    assert {(c["routes"][0], c["spike"] > 0) for c in cases.ATTN_SPIKE_CASES} == {("FWD_PS", True), ("FWD_PS", False), ("FWD_ASM", True), ("FWD_ASM", False)}


def test_thresholds_between_the_routes(K):
    name = lambda Nq, Nk, mask=None, **kw: K.attn_route_names(Nq, Nk, 64, BF, mask or K.Mask(), **kw)
    ps = dict(q_prescaled=True)
    assert name(128, 128, **ps) == ("FWD_ASM", "DQ_ASM", "DKDV_ASM") and name(128, 256, **ps)[2] == "DKDVW_ASM"
    assert name(127, 128, **ps) == ("FWD_PS", "DQ_PS", "DKDV_PS") and name(64, 128, **ps) == ("FWD_PS", "DQ_PS", "DKDV_ASM")
    assert name(128, 127, **ps) == ("FWD_PS", "DQ_PS", "DKDV_PS") and name(128, 64, **ps) == ("FWD_ASM", "DQ_ASM", "DKDV_PS")
    blk = lambda c, q_off=0, k_off=0: K.Mask(K.MASK_BLOCK_CAUSAL, c, q_off, k_off)
    assert name(256, 256, blk(128), **ps) == ("FWD_ASM", "DQ_ASM", "DKDV_ASM") and name(256, 256, blk(256), **ps)[2] == "DKDVW_ASM"
    assert name(256, 256, blk(64), **ps) == name(256, 256, blk(128, 128, 0), **ps) == name(256, 256, blk(128, 0, 128), **ps) == ("FWD_PS", "DQ_PS", "DKDV_PS")
    assert name(256, 256, K.Mask(K.MASK_CAUSAL), **ps) == name(256, 256, K.Mask(K.MASK_KEYPAD), **ps) == ("FWD_PS", "DQ_PS", "DKDV_PS")
    assert name(32, 1024) == ("FWD_FEWQ", "DQ_FEWQ", "DKDV_GENERIC") == name(1, 5000)
    assert name(33, 1024) == name(32, 1023) == name(32, 1024, K.Mask(K.MASK_CAUSAL)) == name(32, 1024, dropout=True) == ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC")
    assert name(1024, 1024, rope=True) == ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC")
    assert K.attn_route_names(32, 1024, 32, BF) == K.attn_route_names(32, 1024, 64, F32) == ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC")


def test_route_query_refuses_what_the_launch_refuses(K):
    from frankenstein_amd import _lib
    q = lambda *a: _lib.lib().fk_attn_route(*a, None, None, None)
    assert q(128, 128, 64, _lib.FK_BF16, 0, 0, 0, 0, 1, 0, 0) == 0                        # the outputs are optional
    assert q(128, 128, 24, _lib.FK_BF16, 0, 0, 0, 0, 0, 0, 0) == -1                       # head_dim
    assert q(128, 128, 128, _lib.FK_F32, 0, 0, 0, 0, 0, 0, 0) == -1
    assert q(128, 128, 32, _lib.FK_BF16, 0, 0, 0, 0, 1, 0, 0) == -1                       # pre-scaled: bf16, D = 64 only
    assert q(128, 128, 64, _lib.FK_BF16, 5, 0, 0, 0, 1, 0, 0) == -1                       # dense mask / dropout with it
    assert q(128, 128, 64, _lib.FK_BF16, 0, 0, 0, 0, 1, 1, 0) == -1
    assert q(128, 128, 64, _lib.FK_BF16, 2, 0, 0, 0, 0, 0, 0) == -1                       # block-causal without a block
    assert q(128, 256, 64, _lib.FK_BF16, 0, 0, 0, 0, 0, 0, 1) == -1                       # RoPE in the backward: self-attention
    assert q(0, 128, 64, _lib.FK_BF16, 0, 0, 0, 0, 0, 0, 0) == -1 and q(128, 128, 64, 7, 0, 0, 0, 0, 0, 0, 0) == -1
    with pytest.raises(_lib.FrankenHipError, match="head_dim"):
        K.attn_route(128, 128, 24)


# ----------------------------------------------------------------------------------------------- the inputs do their job
@functools.lru_cache(maxsize=2)
def problem(idx):
    c = ALL[idx]
    inp = AI.make_inputs(c)
    q, k, v, do = (AI.heads(inp[n]) for n in ("q", "k", "v", "do"))
    o, lse, mag_o, P = AI.forward(q, k, v, inp["vis"], inp["scale"])
    return c, inp, (q, k, v, do), (o, lse, mag_o, P)


@pytest.mark.parametrize("idx", range(len(ALL)), ids=[c["id"] for c in ALL])
def test_rounding_model_stays_inside_the_bound(idx):
    c, inp, (q, k, v, do), _ = problem(idx)
    dtype, vis, scale = inp["dtype"], inp["vis"], inp["scale"]
    got = AI.rounding_model(q, k, v, do, vis, scale, dtype)
    o, lse, mag_o, P = AI.forward(q, k, v, vis, scale)
    ref = AI.backward(q, k, v, do, P, got["o"], scale)
    ref.update(o=o, mag_o=mag_o)
    fin = torch.isfinite(lse)
    assert torch.equal(fin, torch.isfinite(got["lse"])) and bool(((got["lse"] - lse)[fin].abs() <= 1e-4 + 1e-4 * lse[fin].abs()).all())
    for name in ("o", "dq", "dk", "dv"):
        f, _ = AI.frac(got[name], ref[name], ref["mag_" + name], dtype)
        print(f"MODEL {name} {c['id']} {f:.3f}")
        assert f <= 1.0, (name, f)


def drop_cells(q, k, v, do, vis, scale, dtype, full):
    """q, do [Nq, D], k, v [Nk, D], vis [Nq, Nk] of one head; full: the head's reference (o, dq, dk, dv and mags).  -> the smallest,
    over the visible cells, of the largest |change| / bound per tensor"""
    Nq, Nk = vis.shape
    worst = {n: float("inf") for n in ("o", "dq", "dk", "dv")}
    for r0 in range(0, Nq, T):
        rows = slice(r0, min(Nq, r0 + T))
        vt = vis[rows]
        js = [j for j in range(0, Nk, T) if bool(vt[:, j:j + T].any())]
        if not js:
            continue
        var = vt[None].repeat(len(js), 1, 1)
        for n, j in enumerate(js):
            var[n, :, j:j + T] = False
        empty = ~var.any(-1)                                                   # rows the cell would leave empty keep it
        var = torch.where(empty[..., None], vt[None], var)
        changed = (var != vt[None]).any(-1).any(-1)
        o0, _, _, P0 = AI.forward(q[rows], k, v, vt, scale)
        b0 = AI.backward(q[rows], k, v, do[rows], P0, o0, scale)
        o1, _, _, P1 = AI.forward(q[rows], k, v, var, scale)
        b1 = AI.backward(q[rows], k, v, do[rows], P1, o1, scale)
        for n, j in enumerate(js):
            if not bool(changed[n]):
                continue
            keys = slice(j, min(Nk, j + T))
            moved = {"o": ((o1[n] - o0).abs() / AI.bound(full["o"][rows], full["mag_o"][rows], dtype)).max(),
                     "dq": ((b1["dq"][n] - b0["dq"]).abs() / AI.bound(full["dq"][rows], full["mag_dq"][rows], dtype)).max(),
                     "dk": ((b1["dk"][n] - b0["dk"])[keys].abs() / AI.bound(full["dk"][keys], full["mag_dk"][keys], dtype)).max(),
                     "dv": ((b1["dv"][n] - b0["dv"])[keys].abs() / AI.bound(full["dv"][keys], full["mag_dv"][keys], dtype)).max()}
            for name, m in moved.items():
                worst[name] = min(worst[name], float(m))
    return worst


@pytest.mark.parametrize("idx", range(len(cases.ATTN_ROUTE_CASES)), ids=[c["id"] for c in cases.ATTN_ROUTE_CASES])
def test_a_dropped_cell_is_a_gross_error(idx):
    c, inp, (q, k, v, do), (o, lse, mag_o, P) = problem(idx)
    dtype, scale = inp["dtype"], inp["scale"]
    full = AI.backward(q, k, v, do, P, o, scale)
    full.update(o=o, mag_o=mag_o)
    vis = inp["vis"].expand(c["B"], c["H"], c["Nq"], c["Nk"])
    worst = {n: float("inf") for n in ("o", "dq", "dk", "dv")}
    for b in range(c["B"]):
        for h in range(c["H"]):
            w = drop_cells(q[b, h], k[b, h], v[b, h], do[b, h], vis[b, h], scale, dtype, {n: t[b, h] for n, t in full.items()})
            worst = {n: min(worst[n], w[n]) for n in worst}
    print("CELL", c["id"], " ".join(f"{n} {x:.1f}" for n, x in worst.items()))
    assert all(x >= 2.0 for x in worst.values()), worst


@pytest.mark.parametrize("idx", range(len(cases.ATTN_ROUTE_CASES)), ids=[c["id"] for c in cases.ATTN_ROUTE_CASES])
def test_a_mask_edge_off_by_one_is_a_gross_error(idx):
    c, inp, (q, k, v, do), (o, lse, mag_o, P) = problem(idx)
    dtype, scale = inp["dtype"], inp["scale"]
    vis = inp["vis"].expand(c["B"], c["H"], c["Nq"], c["Nk"])
    bnd = AI.bound(o, mag_o, dtype)
    ar = torch.arange(c["Nk"])
    a, b = AI.edge_keys(vis)                                                   # the visible key at the edge and the hidden one behind it
    worst = float("inf")
    hide = vis & (ar != a[..., None])
    rows = hide.any(-1) & (a >= 0)                                             # rows that keep a key
    o1 = AI.forward(q, k, v, torch.where(rows[..., None], hide, vis), scale)[0]
    if bool(rows.any()):
        worst = min(worst, float(((o1 - o).abs() / bnd).max(-1).values[rows].min()))
    rows = b >= 0
    o2 = AI.forward(q, k, v, vis | (ar == b[..., None]), scale)[0]
    if bool(rows.any()):
        worst = min(worst, float(((o2 - o).abs() / bnd).max(-1).values[rows].min()))
    print("EDGE", c["id"], f"{worst:.1f}")
    assert worst >= 2.0
