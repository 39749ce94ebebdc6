"""The cases of tests/test_attn_rope_gpu.py (tests/cases.py ATTN_ROPE_CASES: attn_bwd with a rope_table, the inverse rotation fused into
the dQ / dK stores) without a GPU: the kernels every case reaches, what the list must cover, and the conditions under which the GPU file
is worth running.  On the float64 reference alone, for every case,
  * a CPU model of the kernels' documented roundings, which rotates the accumulators and rounds once at the store, stays inside the
    bound (largest 0.91 of it);
  * each defect of DEFECTS (no rotation, the forward rotation, a table row one off, rope_off ignored, the neighbouring pair's angle,
    sample 0's table for every sample, the two middle 4-column groups of every 16 columns exchanged as a wrong half-wave exchange would
    leave them; dv rotated as well) moves dq and dk (dv) by at least 2x the bound in at least one row of every block of 32 rows that has
    any gradient, for every sample and head, and in at least 99 % of such rows overall.
2x: a real kernel's own error is at most 1x the bound and may oppose the defect; at 2x the defect still fails the GPU test.  The angles
(attn_inputs.rope_table) keep |cos| and |sin| above 0.38 and are unrelated between rows, pairs and samples, which is what makes every
one of these defects large in every row."""
import functools

import pytest
import torch

from tests import attn_inputs as AI
from tests import cases

BF, F32 = torch.bfloat16, torch.float32
ALL = cases.ATTN_ROPE_CASES
IDS = [c["id"] for c in ALL]
BLOCK = 32                       # rows per wave in every backward kernel
FLOOR = 2e-5                     # the absolute term of attn_inputs.bound


@pytest.fixture(scope="module")
def K():
    from frankenstein_amd import build
    build.build(verbose=False)
    from frankenstein_amd import kernels
    return kernels


def case_routes(K, c):
    vis, extras = AI.visibility(c)
    return K.attn_route_names(c["Nq"], c["Nk"], c["D"], BF if c["dtype"] == "bf16" else F32, AI.make_mask(K, c, extras, vis, "cpu"),
                              q_prescaled=c["ps"], rope=True)


# ----------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_cases_reach_the_routes_they_name(K, case):
    assert case_routes(K, case) == case["routes"]
    assert case["Nq"] == case["Nk"] <= 512 and case["B"] <= 2 and case["H"] <= 3
    assert case["table"] in ("shared", "sample", "strided") and case["rope_off"] >= 0
    tall, Tc = AI.case_table(case)
    assert Tc == case["rope_off"] + case["Nq"] and tall.shape == (1 if case["table"] == "shared" else case["B"], Tc + AI.ROPE_SLACK, case["D"] // 2, 2)
    assert tall.dtype == F32 and float(tall.abs().min()) >= 0.38
    assert (Tc * case["D"]) % 4 == 0                                  # every sample's table starts on 16 bytes


def _where(pred):
    return [c for c in ALL if pred(c)]


def test_the_list_covers_every_fused_store_and_every_table_form():
    gen = ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC")
    ps = ("FWD_PS", "DQ_PS", "DKDV_PS")
    # bf16 D = 64, pre-scaled: the generated streams at 128 / 256 full and 384 / 512 block-causal, the tile loops under every mask
    want = {(128, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_ASM")), (256, ("none",), ("FWD_ASM", "DQ_ASM", "DKDVW_ASM")),
            (384, ("block", 128), ("FWD_ASM", "DQ_ASM", "DKDV_ASM")), (512, ("block", 256), ("FWD_ASM", "DQ_ASM", "DKDVW_ASM")),
            (192, ("none",), ps), (200, ("block", 8), ps), (333, ("causal",), ps), (256, ("sliced", "block", 128, 512, 512), ps)}
    have = {(c["Nq"], c["mask"], c["routes"]) for c in ALL if c["ps"]}
    assert want <= have, want - have
    assert any(c["Nq"] == 260 and c["mask"][0] == "prefix" and c["routes"] == ps for c in ALL if c["ps"])
    assert any(c["Nq"] == 270 and c["mask"] == ("keypad",) and c["routes"] == ps for c in ALL if c["ps"])
    assert all(c["dtype"] == "bf16" and c["D"] == 64 for c in ALL if c["ps"])
    assert all(c["rope_off"] == 256 for c in ALL if c["mask"][0] == "sliced")          # offsets in the mask and in the table at once
    # bf16 D = 64, not pre-scaled, dense mask: the generic kernels on the swizzled image
    assert _where(lambda c: c["dtype"] == "bf16" and c["D"] == 64 and not c["ps"] and c["mask"][0] == "dense" and c["routes"] == gen)
    # the generic kernels: fp32 D 8 / 16 / 32 / 64, bf16 D 8 / 16 / 32 / 128, ragged, the mask kinds spread among them
    g = _where(lambda c: c["routes"] == gen)
    assert {c["D"] for c in g if c["dtype"] == "f32"} == {8, 16, 32, 64} and {c["D"] for c in g if c["dtype"] == "bf16"} >= {8, 16, 32, 128}
    assert all(c["Nq"] % 32 for c in g) and any(c["Nq"] > 128 for c in g)
    assert {c["mask"][0] for c in g} >= {"causal", "block", "keypad", "prefix"}
    assert all(c["routes"] == gen for c in ALL if not c["ps"])
    # across the table: shared and per-sample, rope_off 0 and odd, on every kernel with a fused store
    for i, names in ((1, ("DQ_PS", "DQ_ASM", "DQ_GENERIC")), (2, ("DKDV_PS", "DKDV_ASM", "DKDVW_ASM", "DKDV_GENERIC"))):
        for r in names:
            on = _where(lambda c: c["routes"][i] == r)
            assert any(c["table"] == "shared" for c in on) and any(c["table"] != "shared" and c["B"] > 1 for c in on), r
            assert any(c["rope_off"] == 0 for c in on) and any(c["rope_off"] % 2 for c in on), r
            assert any(c["B"] > 1 and c["H"] > 1 for c in on), r
    assert any(c["table"] == "strided" and c["B"] > 1 for c in ALL)


def test_route_query_refuses_a_table_on_cross_attention(K):
    """fk_attn_route (and fk_attn_bwd, which asks it) refuses rope with Nq != Nk: the table is read at the row index of dq and dk alike.
    The few-query kernels need Nq <= 32 and Nk >= 1024, so they never meet a table."""
    from frankenstein_amd import _lib
    q = lambda Nq, Nk, rope: _lib.lib().fk_attn_route(Nq, Nk, 64, _lib.FK_BF16, 0, 0, 0, 0, 0, 0, rope, None, None, None)
    assert q(128, 128, 1) == 0 and q(128, 256, 0) == 0 and q(128, 256, 1) == -1 and q(256, 128, 1) == -1
    assert q(32, 1024, 0) == 0 and q(32, 1024, 1) == -1 and q(1024, 1024, 1) == 0
    assert K.attn_route_names(32, 1024, 64, BF) == ("FWD_FEWQ", "DQ_FEWQ", "DKDV_GENERIC")
    with pytest.raises(_lib.FrankenHipError, match="self-attention"):
        K.attn_route(32, 1024, 64, BF, rope=True)


# ----------------------------------------------------------------------------------------------- the reference and its mutants
@functools.lru_cache(maxsize=2)
def problem(idx):
    c = ALL[idx]
    inp = AI.make_inputs(c)
    q, k, v, do = (AI.heads(inp[n]) for n in ("q", "k", "v", "do"))
    o, lse, mag_o, P = AI.forward(q, k, v, inp["vis"], inp["scale"])
    tall, Tc = AI.case_table(c)
    return c, inp, (q, k, v, do), (o, lse, mag_o, P), tall, Tc


def rotate_model(x, table, off, dtype):
    """the store of the kernels: fp32 accumulators rotated in fp32 arithmetic, rounded once"""
    N = x.shape[2]
    t = table[:, None, off:off + N]
    c, s = t[..., 0], t[..., 1]
    x0, x1 = x.float()[..., 0::2], x.float()[..., 1::2]
    out = torch.stack([x0 * c + x1 * s, -x0 * s + x1 * c], -1).flatten(-2)
    return AI.bf16(out) if dtype == BF else out.double()


@pytest.mark.parametrize("idx", range(len(ALL)), ids=IDS)
def test_rounding_model_stays_inside_the_bound(idx):
    c, inp, (q, k, v, do), (o, lse, mag_o, P), tall, Tc = problem(idx)
    dtype, vis, scale, off = inp["dtype"], inp["vis"], inp["scale"], c["rope_off"]
    got = AI.rounding_model(q, k, v, do, vis, scale, dtype, store=False)
    ref = AI.unrotate_grads(AI.backward(q, k, v, do, P, got["o"], scale), tall[:, :Tc], off)
    for name in ("dq", "dk"):
        got[name] = rotate_model(got[name], tall[:, :Tc], off, dtype)
    for name in ("dq", "dk", "dv"):
        f, _ = AI.frac(got[name], ref[name], ref["mag_" + name], dtype)
        print(f"MODEL {name} {c['id']} {f:.3f}")
        assert f <= 1.0, (name, f)


def swap_middle_groups(x):
    """columns 4 .. 7 and 8 .. 11 of every 16 exchanged: the store whose half-waves exchanged the wrong registers"""
    g = x.unflatten(-1, (-1, 4, 4))
    return g[..., [0, 2, 1, 3], :].flatten(-3)


# name -> (applies to the case?, mutant of (raw gradient, its mag, tall table, rope_off, Tc) -> what the defective store would write)
DEFECTS = {
    "no_rotation": (lambda c: True, lambda x, m, t, off, Tc: x),
    "forward_rotation": (lambda c: True, lambda x, m, t, off, Tc: AI.unrotate(x, m, t * torch.tensor([1.0, -1.0]), off)[0]),
    "row_plus_1": (lambda c: True, lambda x, m, t, off, Tc: AI.unrotate(x, m, t, off + 1)[0]),
    "row_minus_1": (lambda c: c["rope_off"] > 0, lambda x, m, t, off, Tc: AI.unrotate(x, m, t, off - 1)[0]),
    "rope_off_ignored": (lambda c: c["rope_off"] > 0, lambda x, m, t, off, Tc: AI.unrotate(x, m, t, 0)[0]),
    "pair_xor_1": (lambda c: True, lambda x, m, t, off, Tc: AI.unrotate(x, m, t.unflatten(2, (-1, 2)).flip(3).flatten(2, 3), off)[0]),
    "pair_plus_1": (lambda c: True, lambda x, m, t, off, Tc: AI.unrotate(x, m, t.roll(-1, 2), off)[0]),
    "sample_0_table": (lambda c: c["table"] != "shared", lambda x, m, t, off, Tc: AI.unrotate(x, m, t[:1], off)[0]),
    "middle_groups_exchanged": (lambda c: c["D"] >= 16, lambda x, m, t, off, Tc: swap_middle_groups(AI.unrotate(x, m, t, off)[0])),
}


def gross(mut, ref, mag, dtype, samples=slice(None)):
    """-> (every block of BLOCK rows with a gradient, in every sample and head, has a row the mutant moves by >= 2x the bound; the share
    of such rows among the rows with a gradient).  A row has a gradient when some element of the reference exceeds FLOOR, the absolute
    term of the bound: below it the bound itself cannot tell the row from zero (fully masked rows, keys no query sees, and the few
    keys of a block-causal tail whose whole column of P sums to 1e-6), whatever is done to it."""
    moved = ((mut - ref).abs() >= 2.0 * AI.bound(ref, mag, dtype)).any(-1)[samples]            # [B, H, N]
    live = (ref.abs() > FLOOR).any(-1)[samples]
    assert float(live.sum()) >= 0.9 * float((mag > 0).any(-1)[samples].sum())                  # and those are nearly all rows
    pad = -live.shape[-1] % BLOCK
    blk = lambda t: torch.nn.functional.pad(t, (0, pad)).unflatten(-1, (-1, BLOCK)).any(-1)
    every_block = bool((blk(moved & live) == blk(live)).all())
    return every_block, float((moved & live).sum()) / float(live.sum())


@pytest.mark.parametrize("idx", range(len(ALL)), ids=IDS)
def test_every_defect_of_the_fused_store_is_a_gross_error(idx):
    c, inp, (q, k, v, do), (o, lse, mag_o, P), tall, Tc = problem(idx)
    dtype, scale, off = inp["dtype"], inp["scale"], c["rope_off"]
    raw = AI.backward(q, k, v, do, P, o, scale)
    ref = AI.unrotate_grads(raw, tall[:, :Tc], off)
    tall64 = tall.double()
    bad = []
    for name, (applies, mutant) in DEFECTS.items():
        if not applies(c):
            continue
        samples = slice(1, None) if name == "sample_0_table" else slice(None)        # sample 0 has its own table either way
        for g in ("dq", "dk"):
            ok, share = gross(mutant(raw[g], raw["mag_" + g], tall64, off, Tc), ref[g], ref["mag_" + g], dtype, samples)
            print(f"DEFECT {name} {g} {c['id']} every block {ok} share {share:.4f}")
            if not (ok and share >= 0.99):
                bad.append((name, g, ok, share))
    ok, share = gross(AI.unrotate(raw["dv"], raw["mag_dv"], tall64[:, :Tc], off)[0], ref["dv"], ref["mag_dv"], dtype)
    print(f"DEFECT dv_rotated dv {c['id']} every block {ok} share {share:.4f}")
    if not (ok and share >= 0.99):
        bad.append(("dv_rotated", "dv", ok, share))
    assert not bad, bad


def test_the_reference_rotation_inverts_the_forward_rotation():
    """unrotate is the transpose of the rotation the projection applies (out0 = x0 c - x1 s, out1 = x0 s + x1 c): <R x, g> = <x, R^T g>"""
    t = AI.rope_table(2, 9 + 3, 8, 5)
    g = torch.Generator().manual_seed(3)
    x, gr = torch.randn(2, 2, 9, 8, generator=g, dtype=torch.float64), torch.randn(2, 2, 9, 8, generator=g, dtype=torch.float64)
    cs = t.double()[:, None, 3:12]
    c, s = cs[..., 0], cs[..., 1]
    rx = torch.stack([x[..., 0::2] * c - x[..., 1::2] * s, x[..., 0::2] * s + x[..., 1::2] * c], -1).flatten(-2)
    un, mag = AI.unrotate(gr, gr.abs(), t, 3)
    assert torch.allclose((rx * gr).sum(), (x * un).sum(), rtol=1e-12, atol=1e-12)
    assert bool((un.abs() <= mag + 1e-15).all())
