"""The cases of tests/test_attn_drop_gpu.py (tests/cases.py ATTN_DROP_CASES: attn_fwd and attn_bwd with a dropout tuple) without a GPU:
the kernels every case reaches, what the list must cover, and the conditions under which the GPU file is worth running.  No dropout
mask is stored: the forward, the dQ and the dK/dV kernel each rebuild every keep decision from (b, h, row, key) with index arithmetic of
their own, so the GPU file can only be as sharp as the reference is sensitive to one wrong decision.  On the float64 reference alone
(tests/attn_inputs.py forward / backward with keep = tests/dropout_ref.py's prediction), for every case,
  * a CPU model of the kernels' documented roundings stays inside the bound on o, dq, dk and dv;
  * every mutant of MUTANTS (the mask of key + 1, of row + 1, of a row number built from Nq rounded up to 64, without the head term, with
    b and h exchanged, of the key's index inside its tile of 64, of key + k_off, of another site, of another step, no dropout at all, the
    scale missing, the scale applied twice) moves o, dq, dk and dv by at least 2x the bound somewhere;
  * every backward-only defect (dP not taken through the mask, dV from the undropped P, delta from the undropped O)
    moves the gradients it concerns by at least 2x the bound and leaves o alone;
  * one flipped keep bit moves o by at least 2x the bound at entries in every (query tile, key tile) pair of 64 x 64 the mask leaves
    visible (pairs counted over the case's samples and heads: the kernels' index arithmetic inside a tile pair is the same for all of
    them) and at every key and row residue mod 64 (56 of 64 under a dense mask, whose hidden band and dead rows take residues away),
    for kept bits on every case, for dropped bits on every case with p >= 0.25.
The row-number case (B H Nq > 2^16) adds a mutant confined to its last rows: the row number truncated to 16 bits.
2x: a real kernel's own error is at most 1x the bound and may oppose the defect; at 2x the defect still fails the GPU test."""
import functools

import pytest
import torch

from tests import attn_inputs as AI
from tests import cases
from tests.test_attn_rope_cpu import rotate_model

BF, F32 = torch.bfloat16, torch.float32
ALL = cases.ATTN_DROP_CASES
IDS = [c["id"] for c in ALL]
T = AI.TILE
GEN = ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC")
OUT = ("o", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def K():
    from frankenstein_amd import build
    build.build(verbose=False)
    from frankenstein_amd import kernels
    return kernels


def is_rows_case(c):
    return c["B"] * c["H"] * c["Nq"] > cases.ATTN_DROP_ROWS


# ----------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("case", ALL + [cases.ATTN_DROP_GRAPH_CASE], ids=IDS + ["graph-" + cases.ATTN_DROP_GRAPH_CASE["id"]])
def test_cases_reach_the_generic_kernels(K, case):
    vis, extras = AI.visibility(case)
    mask = AI.make_mask(K, case, extras, vis, "cpu")
    dtype = BF if case["dtype"] == "bf16" else F32
    rope = "table" in case
    assert K.attn_route_names(case["Nq"], case["Nk"], case["D"], dtype, mask, dropout=True, rope=rope) == GEN == case["routes"]
    assert not case["ps"] and 0.0 < case["p"] < 1.0 and case["step"] != 0 and case["site"] != 0
    assert case["layout"] in ("split", "qkv") and (case["layout"] == "split" or case["Nq"] == case["Nk"])
    assert is_rows_case(case) or (case["Nk"] <= 1152 and case["B"] <= 3 and case["H"] <= 3)
    assert case["H"] > 1 and case["Nq"] % T and case["Nk"] > T                    # what the mutants below rely on
    if rope:
        from frankenstein_amd import engine
        assert engine.attn_bwd_rope_path(True, case["D"]) == "fused" and case["Nq"] == case["Nk"] and case["table"] in ("shared", "sample")


def _where(pred):
    return [c for c in ALL if pred(c)]


def test_the_list_covers_every_type_mask_layout_and_probability():
    assert all(c["routes"] == GEN for c in ALL) and len({c["id"] for c in ALL}) == len(ALL)
    # fp32 D 8 / 16 / 32 / 64, bf16 D 8 / 16 / 32 / 64 / 128
    for dtype, D in [("f32", d) for d in (8, 16, 32, 64)] + [("bf16", d) for d in (8, 16, 32, 64, 128)]:
        assert _where(lambda c: c["dtype"] == dtype and c["D"] == D), (dtype, D)
    # every mask kind, each at some p >= 0.25; sliced with both offsets; dense per head with fully masked rows, and the (1, 1) table
    for kind in ("none", "causal", "block", "sliced", "prefix", "keypad", "dense"):
        assert _where(lambda c: c["mask"][0] == kind and c["p"] >= 0.25), kind
    for c in _where(lambda c: c["mask"][0] == "sliced"):
        assert c["mask"][3] - c["Nq"] > 0 and c["mask"][4] - c["Nk"] > 0, c["id"]
    per_head = _where(lambda c: c["mask"][0] == "dense" and c["mask"][2] == c["H"] > 1)
    assert per_head and _where(lambda c: c["mask"] == ("dense", 1, 1))
    for c in per_head:
        assert bool((~AI.visibility(c)[0].any(-1)).any()), c["id"]
    # ragged both ways, Nq != Nk, more than one workgroup of 128 rows (forward, dQ) and of 128 keys (dK/dV), B > 1 and H > 1 together
    assert _where(lambda c: c["Nq"] % T and c["Nk"] % T and c["Nq"] != c["Nk"])
    assert _where(lambda c: c["Nq"] > 128 and c["Nk"] > 128 and c["B"] > 1 and c["H"] > 1)
    # the probabilities
    for p in (0.1, 0.25, 0.5, 0.9):
        assert _where(lambda c: c["p"] == p), p
    # the engine's call in both dtypes: causal, D = 64, ragged N above 256, q | k | v of one buffer
    for dtype in ("bf16", "f32"):
        assert _where(lambda c: c["dtype"] == dtype and c["layout"] == "qkv" and c["mask"] == ("causal",) and c["D"] == 64
                      and c["Nq"] == c["Nk"] > 256 and c["Nq"] % T and "table" not in c), dtype
    assert len(_where(lambda c: c["layout"] == "qkv")) >= 2 and _where(lambda c: c["layout"] == "split")
    # dropout with the fused inverse RoPE: bf16 and fp32, a shared and a per-sample table, a table offset
    rope = _where(lambda c: "table" in c)
    assert {c["dtype"] for c in rope} == {"bf16", "f32"} and {c["table"] for c in rope} == {"shared", "sample"}
    assert any(c["rope_off"] > 0 for c in rope) and any(c["table"] == "sample" and c["B"] > 1 for c in rope)
    # row numbers past 2^16
    assert _where(is_rows_case)


# ----------------------------------------------------------------------------------------------- the reference
def finish(c, g):
    """the gradients as the GPU file compares them: un-rotated on the RoPE cases"""
    if "table" not in c:
        return g
    tall, Tc = AI.case_table(c)
    return AI.unrotate_grads(g, tall[:, :Tc], c["rope_off"])


@functools.lru_cache(maxsize=2)
def problem(idx):
    c = ALL[idx]
    inp = AI.make_inputs(c)
    q, k, v, do = (AI.heads(inp[n]) for n in ("q", "k", "v", "do"))
    keep, s = AI.case_keep(c), AI.drop_scale32(c["p"])
    o, lse, mag_o, P = AI.forward(q, k, v, inp["vis"], inp["scale"], keep, s)
    ref = finish(c, AI.backward(q, k, v, do, P, o, inp["scale"], keep, s))
    ref.update(o=o, mag_o=mag_o)
    return c, inp, (q, k, v, do), keep, s, P, lse, ref


def test_the_scale_is_the_devices():
    """fp32(1) / (fp32(1) - fp32(p)), the value set_dropout stores (csrc/attention.hip), not the float64 quotient"""
    assert AI.drop_scale32(0.5) == 2.0 and AI.drop_scale32(0.1) != 1.0 / 0.9 and abs(AI.drop_scale32(0.1) - 1.0 / 0.9) < 1e-6
    assert torch.equal(torch.tensor(AI.drop_scale32(0.9)).float().double(), torch.tensor(AI.drop_scale32(0.9)).double())


@pytest.mark.parametrize("idx", range(len(ALL)), ids=IDS)
def test_rounding_model_stays_inside_the_bound(idx):
    c, inp, (q, k, v, do), keep, s, P, lse, _ = problem(idx)
    dtype, vis, scale = inp["dtype"], inp["vis"], inp["scale"]
    got = AI.rounding_model(q, k, v, do, vis, scale, dtype, store="table" not in c, keep=keep, drop_scale=s)
    if "table" in c:
        tall, Tc = AI.case_table(c)
        for name in ("dq", "dk"):
            got[name] = rotate_model(got[name], tall[:, :Tc], c["rope_off"], dtype)
    o, _, mag_o, _ = AI.forward(q, k, v, vis, scale, keep, s)
    ref = finish(c, AI.backward(q, k, v, do, P, got["o"], scale, keep, s))
    ref.update(o=o, mag_o=mag_o)
    fin = torch.isfinite(lse)
    assert torch.equal(fin, torch.isfinite(got["lse"])) and bool(((got["lse"] - lse)[fin].abs() <= 1e-4 + 1e-4 * lse[fin].abs()).all())
    assert torch.equal(lse, AI.forward(q, k, v, vis, scale)[1])                   # the statistics do not see the dropout
    for name in OUT:
        f, _ = AI.frac(got[name], ref[name], ref["mag_" + name], dtype)
        print(f"MODEL {name} {c['id']} {f:.3f}")
        assert f <= 1.0, (name, f)


def test_some_row_loses_every_visible_key():
    """allowed: o = 0 with a finite lse (the softmax had keys, the dropout took them all)"""
    found = []
    for idx, c in enumerate(ALL):
        if c["p"] < 0.9:
            continue
        c, inp, _, keep, s, P, lse, ref = problem(idx)
        rows = inp["vis"].expand_as(keep).any(-1) & ~(inp["vis"] & keep).any(-1)
        if bool(rows.any()):
            assert bool(torch.isfinite(lse[rows]).all()) and float(ref["o"][rows].abs().max()) == 0.0
            found.append(c["id"])
    assert found


# ----------------------------------------------------------------------------------------------- mutants of the mask
def run(c, inp, ops, keep, s):
    q, k, v, do = ops
    o, _, _, P = AI.forward(q, k, v, inp["vis"], inp["scale"], keep, s)
    g = finish(c, AI.backward(q, k, v, do, P, o, inp["scale"], keep, s))
    g["o"] = o
    return g


def moved(got, ref, dtype):
    return {n: float(((got[n] - ref[n]).abs() / AI.bound(ref[n], ref["mag_" + n], dtype)).max()) for n in OUT}


def k_off_of(c):
    return c["mask"][4] - c["Nk"]


# name -> (applies to the case?, case -> (keep, scale factor on the case's s, or None for s = 1))
MUTANTS = {
    "key_plus_1": (lambda c: True, lambda c: (AI.case_keep(c, lo=lambda key: key + 1), 1.0)),
    "row_plus_1": (lambda c: True, lambda c: (AI.case_keep(c, hi=lambda b, h, q: (b * c["H"] + h) * c["Nq"] + q + 1), 1.0)),
    "nq_rounded_up": (lambda c: True, lambda c: (AI.case_keep(c, hi=lambda b, h, q: (b * c["H"] + h) * (-(-c["Nq"] // T) * T) + q), 1.0)),
    "no_head_term": (lambda c: True, lambda c: (AI.case_keep(c, hi=lambda b, h, q: (b * c["H"] + 0 * h) * c["Nq"] + q), 1.0)),
    "b_h_swapped": (lambda c: c["B"] > 1, lambda c: (AI.case_keep(c, hi=lambda b, h, q: (h * c["B"] + b) * c["Nq"] + q), 1.0)),
    "key_inside_its_tile": (lambda c: True, lambda c: (AI.case_keep(c, lo=lambda key: key % T), 1.0)),
    "key_plus_k_off": (lambda c: c["mask"][0] == "sliced", lambda c: (AI.case_keep(c, lo=lambda key: key + k_off_of(c)), 1.0)),
    "site_plus_1": (lambda c: True, lambda c: (AI.case_keep(c, site=c["site"] + 1), 1.0)),
    "step_plus_1": (lambda c: True, lambda c: (AI.case_keep(c, step=c["step"] + 1), 1.0)),
    "no_dropout": (lambda c: True, lambda c: (None, None)),
    "scale_missing": (lambda c: True, lambda c: (AI.case_keep(c), None)),
    "scale_twice": (lambda c: True, lambda c: (AI.case_keep(c), AI.drop_scale32(c["p"]))),
    "row_16_bits": (is_rows_case, lambda c: (AI.case_keep(c, hi=lambda b, h, q: ((b * c["H"] + h) * c["Nq"] + q) & 0xFFFF), 1.0)),
}


@pytest.mark.parametrize("idx", range(len(ALL)), ids=IDS)
def test_every_wrong_mask_is_a_gross_error(idx):
    c, inp, ops, keep, s, P, lse, ref = problem(idx)
    bad = []
    for name, (applies, mutant) in MUTANTS.items():
        if not applies(c):
            continue
        mkeep, f = mutant(c)
        assert mkeep is None or f is None or f != 1.0 or not torch.equal(mkeep, keep), name
        if name == "row_16_bits":                                      # confined to the rows at and past 2^16
            rows = (mkeep != keep).any(-1).flatten()
            assert bool(rows[cases.ATTN_DROP_ROWS:].any()) and not bool(rows[:cases.ATTN_DROP_ROWS].any())
        m = moved(run(c, inp, ops, mkeep, 1.0 if f is None else s * f), ref, inp["dtype"])
        print(f"MUTANT {name} {c['id']} " + " ".join(f"{n} {x:.1f}" for n, x in m.items()))
        if not all(x >= 2.0 for x in m.values()):
            bad.append((name, m))
    assert not bad, bad


@pytest.mark.parametrize("idx", range(len(ALL)), ids=IDS)
def test_every_backward_only_defect_is_a_gross_error(idx):
    """dP not through the mask: dS = P (dO V^T - delta) (dq, dk); dV from the undropped P (dv); delta from the undropped O (dq, dk)"""
    c, inp, (q, k, v, do), keep, s, P, lse, ref = problem(idx)
    dtype, scale = inp["dtype"], inp["scale"]
    plain = finish(c, AI.backward(q, k, v, do, P, ref["o"], scale))
    o_eval = AI.forward(q, k, v, inp["vis"], scale)[0]
    delta = finish(c, AI.backward(q, k, v, do, P, o_eval, scale, keep, s))
    m = lambda got, n: float(((got[n] - ref[n]).abs() / AI.bound(ref[n], ref["mag_" + n], dtype)).max())
    got = {"dp_unmasked dq": m(plain, "dq"), "dp_unmasked dk": m(plain, "dk"), "dv_undropped dv": m(plain, "dv"),
           "delta_undropped dq": m(delta, "dq"), "delta_undropped dk": m(delta, "dk")}
    print(f"BACKWARD {c['id']} " + " ".join(f"{n} {x:.1f}" for n, x in got.items()))
    assert all(x >= 2.0 for x in got.values()), got
    assert torch.equal(delta["dv"], ref["dv"])                         # dv does not read delta


# ----------------------------------------------------------------------------------------------- one wrong decision
def single_bit(c, inp, v, keep, s, P, ref):
    """-> bool [B, H, Nq, Nk]: flipping the keep bit of (row, key) alone moves o by at least 2x the bound somewhere in the row.  o is
    linear in keep: the flip changes o[row] by -+ P[row, key] s v[key]."""
    bnd = AI.bound(ref["o"], ref["mag_o"], inp["dtype"])
    out = torch.zeros_like(keep)
    for b in range(c["B"]):
        for h in range(c["H"]):
            step = (P[b, h] * s)[:, :, None] * v[b, h].abs()[None, :, :]              # [Nq, Nk, D]
            out[b, h] = ((step / bnd[b, h][:, None, :]).max(-1).values >= 2.0)
    return out & inp["vis"].expand_as(keep)


@pytest.mark.parametrize("idx", range(len(ALL)), ids=IDS)
def test_one_flipped_keep_bit_is_a_gross_error_in_every_tile_pair_and_residue(idx):
    c, inp, (q, k, v, do), keep, s, P, lse, ref = problem(idx)
    Nq, Nk = c["Nq"], c["Nk"]
    sens = single_bit(c, inp, v, keep, s, P, ref)
    vis = inp["vis"].expand_as(keep)
    # the linear step is what a real flip does: one kept and one dropped entry, recomputed
    for bits in (sens & keep, sens & ~keep):
        b, h, i, j = (int(x) for x in bits.nonzero()[len(bits.nonzero()) // 2])
        flipped = keep.clone()
        flipped[b, h, i, j] = ~flipped[b, h, i, j]
        o1 = AI.forward(q[b, h, i:i + 1], k[b, h], v[b, h], vis[b, h, i:i + 1], inp["scale"], flipped[b, h, i:i + 1], s)[0]
        assert float(((o1[0] - ref["o"][b, h, i]).abs() / AI.bound(ref["o"][b, h, i], ref["mag_o"][b, h, i], inp["dtype"])).max()) >= 2.0
    pad = lambda t: torch.nn.functional.pad(t, (0, -Nk % T, 0, -Nq % T))
    pairs = lambda t: pad(t).unflatten(-1, (-1, T)).unflatten(-3, (-1, T)).any(-1).any(-2).any(0).any(0)      # [query tiles, key tiles]
    floor = 56 if c["mask"][0] == "dense" else T
    for name, bits in (("kept", sens & keep), ("dropped", sens & ~keep)):
        n = int(bits.sum())
        missing = int((pairs(vis) & ~pairs(bits)).sum())
        keys = len({int(j) % T for j in bits.any(0).any(0).any(0).nonzero().flatten()})
        rows = len({int(i) % T for i in bits.any(0).any(0).any(-1).nonzero().flatten()})
        print(f"BIT {name} {c['id']} entries {n} tile pairs without one {missing} of {int(pairs(vis).sum())} key residues {keys} row residues {rows}")
        if name == "kept" or c["p"] >= 0.25:
            assert missing == 0 and keys >= min(floor, Nk) and rows >= min(floor, Nq), (name, n, missing, keys, rows)
        assert n > 0
