"""The sampler's float64 restatement (tests/sample_ref.py) and its table of cases (tests/sample_cases.py), checked without a GPU, so that
tests/test_sample_draws_gpu.py is known to be able to fail:

  distribution    over a fine grid of u the reference's token reproduces the renormalised softmax over the kept set, to one grid step a token
  ambiguous share for every case and the (seed, step, rows) it uses at most 5 % of the draws have more than one accepted token: a condition
                  on the inputs (a case that misses it is reshaped, the cap stays)
  fp32 emulation  the kernel's summation order in fp32 (chunk sums, Hillis-Steele scan, the winner's walk, its fallbacks) stays inside the
                  accepted set on every draw of every case: EPS leaves room for the arithmetic it was derived for
  defects         fifteen ways a kernel can be wrong, each applied to the restatement, each puts >= 5 % of the draws of its named case outside
                  the accepted set

Ambiguous shares measured here (2 steps x B rows per case; `-s` prints them): 0 % wherever a crop or a nucleus leaves at most a few dozen
tokens and at V <= 37; v1000-normal 1.75, v1000-ninf 2.14, v1024-normal-bigstep 0.97, v1024-placed-k40 0.19, v1024-x4-kV+5 0.97,
v1025-normal 1.17, v1025-placed 2.14, v1025-ninf-kV-1 1.56, v50257-x4 2.33, v50257-placed 4.28, v50257-ninf-kV-1 2.53,
v50257-ties-k8 0.19, v50257-kV 1.75 %.  The fp32 emulation's largest excursion is 0.010 (v50257-placed)."""
import numpy as np
import pytest

from tests import sample_cases as SC
from tests import sample_ref as R

f32 = np.float32
CAP = 0.05


@pytest.fixture(scope="module", params=SC.CASES, ids=lambda c: c.name)
def loaded(request):
    """(case, logits, RowRef per row, u per launch and row); module scope, so the tests of one case run next to each other and share it"""
    case = request.param
    rows = SC.logits_of(case)
    return case, rows, SC.refs_of(case, rows), [SC.uniforms_of(case, n) for n in range(SC.LAUNCHES)]


# =============================================================================================== the restatement itself
def test_philox_known_answers():
    """the known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10 rounds)"""
    assert R.philox4x32_10((0, 0), (0, 0, 0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert R.philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_uniform_reads_every_word_of_seed_step_and_row():
    u = R.uniform(SC.SEED_HI, SC.STEP_BIG, 7)
    assert 0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24)
    assert u == (R.philox4x32_10((0x9ABCDEF0, 0x12345678), (5, 1, 7, 0x5A3C))[0] >> 8) / 2 ** 24
    others = [R.uniform(SC.SEED_HI & R.M32, SC.STEP_BIG, 7), R.uniform(SC.SEED_HI, 5, 7), R.uniform(SC.SEED_HI, SC.STEP_BIG, 8)]
    assert len({u, *others}) == 4
    assert R.uniform(-1, -1, 0) == R.uniform(2 ** 64 - 1, 2 ** 64 - 1, 0)          # the int64 the state holds, read as the device reads it


def test_draw_on_a_row_worked_by_hand():
    """p = .1 .2 0 .3 .4 (index 2 at -inf): boundaries at .1 .3 .3 .6"""
    row = np.log(np.array([0.1, 0.2, 1.0, 0.3, 0.4])).astype(f32)
    row[2] = -np.inf
    for u, want in ((0.0, 0), (0.0999, 0), (0.1001, 1), (0.2999, 1), (0.3001, 3), (0.5999, 3), (0.6001, 4), (1 - 2.0 ** -24, 4)):
        w, acc, exc = R.draw(row, 1.0, None, 1.0, u)
        assert w == want and acc.tolist() == [want] and exc(want) == 0.0, u
        assert exc(2) == np.inf and exc(5) == np.inf and exc(-1) == np.inf
    # on a boundary both neighbours are accepted, the entry without mass between them never
    r = R.row_ref(row, 1.0, None)
    u = float(r.cdf[1] / r.total)
    assert r.accepted(u).tolist() == [1, 3] and int(r.n_accepted(u)) == 2
    assert r.accepted(u + 0.9 * R.EPS).tolist() == [1, 3] and r.accepted(u + 1.1 * R.EPS).tolist() == [3]
    assert abs(float(r.excursion(1, u + 3 * R.EPS)) - 3.0) < 1e-6 and float(r.excursion(3, u + 3 * R.EPS)) == 0.0
    # top_k = 2 keeps .3 and .4 only; T scales in fp32
    w, acc, _ = R.draw(row, 1.0, 2, 1.0, 0.42)
    assert w == 3 and R.kept(row, 1.0, 2).tolist() == [False, False, False, True, True]
    assert R.draw(row, 1.0, 2, 1.0, 0.43)[0] == 4                                  # .3 / .7 = .4286
    ties = np.array([1.0, 3.0, 2.0, 2.0, 0.0, 2.0], f32)
    assert R.kept(ties, 0.7, 2).tolist() == [False, True, True, True, False, True]  # ties with the second largest all stay
    assert R.kept(ties, 0.7, 6).all() and R.kept(ties, 0.7, 0).all() and R.kept(ties, 0.7, None).all() and R.kept(ties, 0.7, 9).all()
    bad, n_amb, worst = R.judge([r, r, r], [0.05, 0.2, u], [0, 3, 3])
    assert [b[0] for b in bad] == [1] and n_amb == 1 and worst > 1.0
    with pytest.raises(AssertionError, match="outside the accepted set"):
        R.assert_draws([r], [0.2], [0])


def test_kept_refuses_a_nucleus_row_without_margin():
    row = np.log(np.array([0.5, 0.3, 0.2])).astype(f32)
    assert R.kept(row, 1.0, None, 0.65).tolist() == [True, True, False]
    with pytest.raises(AssertionError, match="margin"):
        R.kept(row, 1.0, None, 0.51)


def test_the_table_covers_every_value_of_every_axis():
    cs = SC.CASES
    assert 20 <= len(cs) <= 30
    assert {c.V for c in cs} == {1, 37, 1000, 1024, 1025, 50257}
    assert {c.T for c in cs} == {1.0, 0.7, 1.3} and {c.top_p for c in cs} == {1.0, 0.45, 0.70}
    assert {c.seed for c in cs} == {SC.SEED_LO, SC.SEED_HI} and SC.SEED_LO < 2 ** 32 and 2 ** 32 <= SC.SEED_HI < 2 ** 63
    assert {c.step for c in cs} == {0, 1, 2 ** 32 + 5}
    assert {c.B for c in cs} == {1, 257}
    for V in (37, 1000, 1025, 50257):          # per vocabulary: no crop, a crop, and rows with placed mass
        mine = [c for c in cs if c.V == V]
        assert any(c.top_k is None for c in mine) and any(c.top_k and c.top_k < V for c in mine) and any(c.kind == "placed" for c in mine), V
    assert any(c.top_k == 1 for c in cs) and any(c.top_k == 40 for c in cs)
    assert any(c.top_k == c.V - 1 for c in cs) and any(c.top_k == c.V for c in cs) and any(c.top_k and c.top_k > c.V for c in cs)
    assert any(c.ninf and c.top_k is None for c in cs) and any(c.ninf and c.top_k for c in cs)
    assert R.chunk_of(1000) == 1 and R.chunk_of(1024) == 1 and R.chunk_of(1025) == 2 and R.chunk_of(50257) == 50 and 50257 - 1005 * 50 == 7


def test_the_rows_of_a_case_differ_and_ties_cases_tie(loaded):
    case, rows, refs, _ = loaded
    assert rows.dtype == f32 and rows.shape == (case.B, case.V)
    if case.V > 1:
        assert len({r.tobytes() for r in rows}) == case.B
    if case.kind == "integer":                  # more than 8 stay in most rows: the 8th value repeats
        n_kept = np.array([int(R.kept(r, case.T, case.top_k).sum()) for r in rows])
        assert (n_kept >= 8).all() and (n_kept > 8).mean() > 0.5, n_kept[:16]
    if case.ninf:
        assert np.isneginf(rows[:, -1]).all() and (np.isneginf(rows).sum(1) == 4).all()
        assert not any(bool(r.has_mass(case.V - 1)) for r in refs)
    if case.kind == "placed":
        heavy = {int(i) for r in refs for i in np.nonzero(r.probs() > 0.05)[0]}
        assert heavy <= set(SC.special_positions(case.V)) and {0, case.V - 1} <= heavy and len(heavy) >= min(10, len(SC.special_positions(case.V)) - 1)


# =============================================================================================== distribution
GRID = 1 << 16


def test_want_over_a_grid_of_u_is_the_softmax_over_the_kept_set(loaded):
    case, rows, refs, _ = loaded
    u = np.arange(GRID) / GRID
    for b in sorted({0, 1 % case.B, case.B - 1}):
        keep = R.kept(rows[b], case.T, case.top_k, case.top_p)
        x = (rows[b].astype(np.float64) * float(f32(1.0) / f32(case.T)))[keep]          # the fp32 product differs from this by 2^-24 relative
        p = np.zeros(case.V)
        p[keep] = np.exp(x - x.max()) / np.exp(x - x.max()).sum()
        cnt = np.bincount(refs[b].want(u), minlength=case.V)
        assert cnt.sum() == GRID and cnt[~keep].sum() == 0
        # an interval of length p holds floor(p G) or ceil(p G) grid points; 2^-24 * |x| <= 2e-6 relative on p moves that by under 0.2
        assert np.abs(cnt - p * GRID).max() <= 1.0 + 0.2, (b, np.abs(cnt - p * GRID).max())


# =============================================================================================== ambiguous share
def test_at_most_five_percent_of_the_draws_are_ambiguous(loaded):
    case, rows, refs, us = loaded
    n_amb = sum(int(r.n_accepted(u) > 1) for launch in us for r, u in zip(refs, launch))
    n_none = sum(int(r.n_accepted(u) < 1) for launch in us for r, u in zip(refs, launch))
    share = n_amb / (case.B * len(us))
    print(f"AMBIGUOUS {case.name} {100 * share:.2f} %")
    assert n_none == 0
    assert share <= CAP, share


# =============================================================================================== the kernel's order in fp32
class KernelOrder:
    """sample_topk_kernel's arithmetic behind the crop, in numpy fp32: e = exp(x - mx) per kept entry, per-thread sums of contiguous chunks
    in index order, a Hillis-Steele inclusive scan of the 1024 sums, target = u * total, the thread whose span holds the target walks its
    chunk from the scan's prefix, and the two fallbacks.  numpy's expf stands in for the device's."""

    def __init__(self, logits32, T, top_k, top_p):
        x = R.scaled(logits32, T)
        self.keep = R.kept(logits32, T, top_k, top_p)
        self.V, self.chunk = x.size, R.chunk_of(x.size)
        mx = x[self.keep].max()
        with np.errstate(invalid="ignore"):
            self.e = np.where(self.keep, np.exp((x - mx).astype(f32)), f32(0)).astype(f32)
        pad = np.zeros(R.SAMPLE_THREADS * self.chunk, f32)
        pad[:self.V] = self.e
        pad = pad.reshape(R.SAMPLE_THREADS, self.chunk)
        part = np.zeros(R.SAMPLE_THREADS, f32)
        for j in range(self.chunk):
            part = part + pad[:, j]
        scan, o = part.copy(), 1
        while o < R.SAMPLE_THREADS:
            nxt = scan.copy()
            nxt[o:] = scan[o:] + scan[:-o]
            scan, o = nxt, o * 2
        assert part.dtype == f32 and scan.dtype == f32
        self.part, self.scan, self.total = part, scan, scan[-1]

    def draw(self, u):
        target = f32(u) * self.total                        # (c0 >> 8) * 2^-24 is exact in fp32
        before = np.concatenate(([f32(0)], self.scan[:-1]))
        hit = np.nonzero((self.part > 0) & (before <= target) & (target < self.scan))[0]
        assert hit.size <= 1
        if hit.size:
            t = int(hit[0])
            acc, pick = before[t], -1
            for i in range(t * self.chunk, min(self.V, (t + 1) * self.chunk)):
                if self.keep[i]:
                    acc = f32(acc + self.e[i])
                    if self.e[i] > 0:
                        pick = i
                    if acc > target:
                        break
            return pick
        return int(np.nonzero(self.e > 0)[0][-1])          # target >= total by rounding: the last kept index with mass


def test_the_kernels_order_in_fp32_stays_inside_the_accepted_set(loaded):
    case, rows, refs, us = loaded
    emu = [KernelOrder(r, case.T, case.top_k, case.top_p) for r in rows]
    worst = 0.0
    for launch in us:
        worst = max(worst, R.assert_draws(refs, launch, [k.draw(u) for k, u in zip(emu, launch)], f"{case.name} fp32 emulation"))
    print(f"EMULATION {case.name} largest excursion {worst:.3f}")
    # the extremes of u
    for u in (0.0, 1.0 - 2.0 ** -24):
        R.assert_draws(refs[:8], [u] * min(8, case.B), [k.draw(u) for k in emu[:8]], f"{case.name} fp32 emulation at u = {u}")


# =============================================================================================== defects
def _drop(case, rows, which):
    """references whose kept set lacks the indices `which` (bool [V]): mass the wrong kernel never adds to its CDF"""
    return [R.RowRef(R.scaled(r, case.T), R.kept(r, case.T, case.top_k, case.top_p) & ~which) for r in rows]


def _wrong_u(fn):
    def got(case, rows, refs, launch):
        return [int(r.want(fn(case, case.step + launch, b))) for b, r in enumerate(refs)]
    return got


def _wrong_ref(build):
    def got(case, rows, refs, launch):
        return [int(w.want(u)) for w, u in zip(build(case, rows), SC.uniforms_of(case, launch))]
    return got


def _descending(case, rows, refs, launch):
    out = []
    for r, u in zip(refs, SC.uniforms_of(case, launch)):
        p = r.probs()
        order = np.argsort(-p, kind="stable")
        out.append(int(order[min(np.searchsorted(np.cumsum(p[order]), u, side="right"), case.V - 1)]))
    return out


def _exactly_k(case, rows):
    refs = []
    for r in rows:
        x = R.scaled(r, case.T)
        kth = np.partition(x, x.size - case.top_k)[x.size - case.top_k]
        keep = x > kth
        ties = np.nonzero(x == kth)[0][:case.top_k - int(keep.sum())]          # the lowest indices fill the k places, the other ties go
        keep[ties] = True
        refs.append(R.RowRef(x, keep))
    return refs


def _top_p_of_everything(case, rows):
    refs = []
    for r in rows:
        x = R.scaled(r, case.T)
        everything = R.nucleus_rule(x.astype(np.float64), np.ones(x.size, bool), case.top_p)[0]
        refs.append(R.RowRef(x, R.topk_rule(x, case.top_k) & everything))
    return refs


def _chunk_mask(case, pick):
    i, c = np.arange(case.V), R.chunk_of(case.V)
    return pick(i, c)


# defect -> (the case that catches it, the tokens a kernel with that defect emits)
DEFECTS = {
    "row missing from the counter": ("v1000-normal", _wrong_u(lambda c, s, b: R.uniform(c.seed, s, 0))),
    "step high word dropped": ("v1024-normal-bigstep", _wrong_u(lambda c, s, b: R.uniform(c.seed, s & R.M32, b))),
    "seed high word dropped": ("v1025-normal", _wrong_u(lambda c, s, b: R.uniform(c.seed & R.M32, s, b))),
    "u taken from the low 24 bits": ("v1000-normal", _wrong_u(lambda c, s, b: (R.counter_word(c.seed, s, b) & 0xFFFFFF) / 2 ** 24)),
    "counter constant wrong": ("v37-normal", _wrong_u(lambda c, s, b: (R.counter_word(c.seed, s, b, tag=0x5A3D) >> 8) / 2 ** 24)),
    "last element of every chunk not summed": ("v50257-placed", _wrong_ref(lambda c, rows: _drop(c, rows, _chunk_mask(c, lambda i, k: i % k == k - 1)))),
    "the chunk that V cuts short not summed": ("v1025-placed", _wrong_ref(lambda c, rows: _drop(c, rows, _chunk_mask(c, lambda i, k: i >= (c.V // k) * k)))),
    "one wave's scan contribution lost": ("v50257-x4", _wrong_ref(lambda c, rows: _drop(c, rows, _chunk_mask(c, lambda i, k: (i // k) // 64 == 3)))),
    "CDF in descending-probability order": ("v1000-x4-k40", _descending),
    "token w + 1": ("v50257-k40-bigstep", lambda c, rows, refs, n: [min(int(r.want(u)) + 1, c.V - 1) for r, u in zip(refs, SC.uniforms_of(c, n))]),
    "token w - 1": ("v37-placed-kV-1", lambda c, rows, refs, n: [max(int(r.want(u)) - 1, 0) for r, u in zip(refs, SC.uniforms_of(c, n))]),
    "ties at the k-th value dropped": ("v1000-ties-k8", _wrong_ref(_exactly_k)),
    "temperature ignored": ("v1000-x4-k40", _wrong_ref(lambda c, rows: [R.row_ref(r, 1.0, c.top_k) for r in rows])),
    "top_p applied to the uncropped mass": ("v1000-placed-k5-p70", _wrong_ref(_top_p_of_everything)),
    # NaN sorts above +inf and poisons the sum: no thread's span holds the target, and the fallback emits the last index with mass
    "a column behind V read": ("v1000-normal", lambda c, rows, refs, n: [int(np.nonzero(r.probs() > 0)[0][-1]) for r in refs]),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_defect_is_caught_by_its_named_case(defect):
    name, emits = DEFECTS[defect]
    case = SC.BY_NAME[name]
    rows = SC.logits_of(case)
    refs = SC.refs_of(case, rows)
    outside = 0
    for launch in range(SC.LAUNCHES):
        us = SC.uniforms_of(case, launch)
        outside += len(R.judge(refs, us, emits(case, rows, refs, launch))[0])
    share = outside / (case.B * SC.LAUNCHES)
    print(f"DEFECT {defect!r} on {name}: {100 * share:.1f} % of the draws outside the accepted set")
    assert share >= 0.05, share


def test_the_defect_list_is_the_issues():
    assert len(DEFECTS) == 15 and all(name in SC.BY_NAME for name, _ in DEFECTS.values())
