"""The table of tests/head_ce_cases.py pinned without a GPU: the operands are exact, every vocabulary column (every 64-column part at
V = 50257) carries at least 10 x the lse bound in some valid row, each case reaches the paths of csrc/head_ce.hip its comment in
tests/test_head_ce_gpu.py claims (computed from BM = BN = 128, BK = 64 / 32 and 64-column parts: a changed tile size fails here instead of
turning a case into a copy of another), and the check functions the GPU test uses accept the kernel's arithmetic restated in fp32 on
the CPU and reject each of nine planted mistakes."""
import pytest
import torch

from tests import head_ce_cases as C

F32, BF16 = C.F32, C.BF16
DT = [F32, BF16]


def dtid(d):
    return "bf16" if d == BF16 else "fp32"


@pytest.mark.parametrize("dtype", DT, ids=dtid)
@pytest.mark.parametrize("shape", C.CASES, ids=C.cid)
def test_operands_exact_and_every_column_matters(shape, dtype):
    c = C.make(shape, dtype)                                       # asserts the exactness of operands and logits
    r = c.ref
    assert c.h.stride(0) == c.K + 8 and c.w.stride(0) == c.K + 8 and c.w.shape[0] == c.path.wrows
    assert bool((c.w[c.V:].float() == C.FILL).all()) and (c.b is None or bool((c.b[c.V:].float() == C.FILL).all()))
    assert float((r.logits.max(-1).values - r.logits.min(-1).values).max()) < 14.0 and 0.7 < float(r.logits.std()) < 2.0
    ratio = C.sensitivity(c)
    print(f"HEADCE {C.cid(shape)} {dtid(dtype)}: sensitivity {ratio:.1f}, e32 lse {r.e_lse:.2e} s {r.e_s:.2e} loss {r.e_loss:.2e}, "
          f"lse bound {float(C.lse_bound(r.e_lse, r.lse).max()):.2e}")
    assert ratio >= 10.0
    tg = c.tg
    for t in (0, c.V - 1) + c.path.edge_targets:
        assert bool(((tg == t) & r.valid).any()), f"no valid row has target {t}"
    assert bool((tg[::7] == -100).all()) and all(int((tg == t).sum()) >= 1 for t in (c.V, c.path.wrows - 1, -1))
    assert r.nvalid == int(((tg >= 0) & (tg < c.V)).sum()) and not bool(r.valid[tg >= c.V].any())
    if c.rows > 65:
        assert bool(r.valid[64:].any())


def test_ignore_index_3_and_all_ignored():
    for dtype in DT:
        c = C.make(C.IGNORE3_CASE, dtype, 3)
        assert int((c.tg == 3).sum()) >= 4 + c.rows // 7 - 1 and not bool(c.ref.valid[c.tg == 3].any())
        assert c.ref.nvalid < C.make(C.IGNORE3_CASE, dtype).ref.nvalid + 32 and bool((c.tg == -1).any())
        z = C.make(C.IGNORE3_CASE, dtype, -100, None, True)
        assert z.ref.nvalid == 0 and z.ref.loss != z.ref.loss and not bool(z.ref.dl.any())


def test_running_maximum_probes():
    rows, V, K = C.SPIKE_CASE
    cols = C.spike_columns(V)
    assert cols[0] < 64 and cols[1] == 64 * 64 - 1 and cols[2] // 64 == C.paths(C.SPIKE_CASE, F32).npart - 1
    for col in cols:
        r = C.make(C.SPIKE_CASE, F32, -100, col).ref
        assert bool((r.logits.argmax(-1) == col).all()) and bool((r.m == r.logits[:, col]).all())
        assert bool((r.s >= 1.0).all()) and bool((r.s <= 1.0 + 1e-6).all())


def test_path_table():
    P = C.paths
    a, b = P((70, 40, 8), F32), P((70, 40, 8), BF16)
    assert (a.npart, a.tiles, a.nk, b.nk, a.pieces, b.pieces) == (1, 1, 1, 1, 2, 1)      # one part of a tile's two; rows 64..69 alone in wm = 1
    a, b = P((128, 64, 64), F32), P((128, 64, 64), BF16)
    assert (a.npart, a.tiles, a.nk, b.nk, a.k_tail, b.k_tail, a.pad, b.pad) == (1, 1, 2, 1, 0, 0, 0, 0)
    a, b = P((129, 129, 72), F32), P((129, 129, 72), BF16)
    assert (a.npart, a.tiles, a.parts_in_last_tile, a.nk, b.nk, a.k_tail, b.k_tail) == (3, 4, 1, 3, 2, 8, 8)
    a, b = P((203, 211, 160), F32), P((203, 211, 160), BF16)
    assert (a.npad, b.npad, 203 % 4, a.nk, b.nk, a.tiles) == (212, 216, 3, 5, 3, 4)
    a = P((66, 4161, 16), F32)
    assert (a.npart, a.npart - 64, a.tiles, a.tiles_mod8) == (66, 2, 33, 1)               # the merge loop's second pass: two lanes
    a, b = P((333, 300, 768), F32), P((333, 300, 768), BF16)
    assert (a.tiles, a.nk, b.nk, a.npart) == (9, 24, 12, 5)
    a = P((70, 50257, 32), BF16)
    assert (a.npart, a.tiles, a.tiles_mod8, a.npad, a.nk) == (786, 393, 1, 50264, 1)
    for shape in C.CASES:
        assert P(shape, F32).edge_targets == tuple(t for t in (63, 64, 127, 128) if t < shape[1])
    assert [C.has_bias(s) for s in C.CASES] == [True, False, True, False, True, False, True]


def _checks(c, o):
    return {"stats": lambda: C.check_stats(c, o.m, o.s, o.t), "lse_loss": lambda: C.check_lse_loss(c, o.lse, o.loss2),
            "dlT": lambda: C.check_dlT(c, o.dlT), "db": lambda: C.check_db(c, o.db)}


def _case(shape, dtype, mutant):
    return C.make(shape, dtype, 3) if mutant == "ignore_minus_100" else C.make(shape, dtype)


@pytest.mark.parametrize("dtype", DT, ids=dtid)
@pytest.mark.parametrize("shape", C.CASES, ids=C.cid)
def test_checks_accept_the_fp32_restatement(shape, dtype):
    extra = [C.make(shape, dtype, 3), C.make(shape, dtype, -100, None, True)] if shape in (C.IGNORE3_CASE, C.IGNORE3_BIAS_CASE) else []
    for c in [C.make(shape, dtype)] + extra:
        for run in _checks(c, C.restate(c)).values():
            run()
    c = C.make(shape, dtype)
    C.check_dlT(c, C.restate(c, vpad=c.V + 1 if c.V % 128 else c.V, rows_pad=-(-c.rows // 4) * 4).dlT)


# which checks a mutant must fail (the others need not see it)
REJECTED_BY = {"column_dropped": ("stats", "lse_loss"), "part_dropped": ("stats", "lse_loss"), "part_twice": ("stats", "lse_loss"),
               "target_plus_one": ("stats", "lse_loss"), "target_next_row": ("stats", "lse_loss", "dlT"), "padding_rows": ("stats", "lse_loss"),
               "ignore_minus_100": ("lse_loss", "dlT", "db"), "dlT_untransposed": ("dlT",), "db_half_tile": ("db",)}


# ignore_index = 3 is passed in one case only
MUTANT_CASES = [(s, m) for s in C.CASES for m in C.MUTANTS if m != "ignore_minus_100" or s == C.IGNORE3_CASE]


@pytest.mark.parametrize("dtype", DT, ids=dtid)
@pytest.mark.parametrize("shape,mutant", MUTANT_CASES, ids=lambda v: C.cid(v) if isinstance(v, tuple) else v)
def test_checks_reject_the_mutants(shape, mutant, dtype):
    c = _case(shape, dtype, mutant)
    checks = _checks(c, C.restate(c, mutant))
    for name in REJECTED_BY[mutant]:
        with pytest.raises(AssertionError):
            checks[name]()


def test_engine_case_and_what_the_bf16_storage_roundings_cost():
    """The engine-level case of tests/test_head_ce_gpu.py: its targets, that LN(x) is exact in bf16 on its inputs (asserted by
    engine_case), and — every product in float64, rounded to bf16 only where engine.HeadCrossEntropy stores bf16 (dlT, dh, dx) — how much
    of the tolerance of test_head_ce_fused_kernels those roundings alone use: at most 3/4 is allowed, so that the storage format leaves a
    quarter to the kernels' fp32 arithmetic (which uses 0.003 of the fp32 tolerance).  Measured: dx 0.25, dln_w 0.50, dln_b 0.40, dW 0.27.
    With a random x, whose LN(x) is rounded inside the engine where the reference cannot follow, the roundings alone came to 1.18 x (dx)
    and 1.25 x (dln_b) the tolerance: no implementation that stores bf16 could have passed."""
    for dtype in DT:
        e = C.engine_case(dtype)
        assert int((e.tg == 3).sum()) > e.tg.numel() // 7 + 2 and e.loss == e.loss and all(bool(torch.isfinite(g).all()) for g in e.grads.values())
        assert bool((e.x.abs().sum(-1) > 0).all()) and float(e.x.sum(-1).abs().max()) == 0.0 and len(set(e.x.abs().flatten().tolist())) == 3
    emu = C.engine_emulation(C.engine_case(BF16))
    print("HEADCE engine emulation:", {k: round(v, 3) for k, v in emu.items()})
    assert all(v < 0.75 for v in emu.values()), emu
