"""The sampler's draw restated in numpy / float64 (no GPU): sample_topk_kernel of csrc/decode.hip, behind fk_sample_topk, fk_sample_topk_eos
and fk_sample_topp, is a pure function of (logits, temperature, top_k, top_p, seed, step, row), and this file is that function.

    x_i   = logits_i * (1.0f / temperature)                       both operations in fp32, so ties at the k-th value are the kernel's
    kept  = x_i >= the k-th largest x (ties kept; top_k <= 0 or >= V: everything), then rules 1-5 of fk_sample_topp for top_p < 1
    e_i   = exp(x_i - max kept), cdf = cumulative sum of e IN INDEX ORDER, total = cdf[V - 1]                     (float64 here)
    u     = (c0 >> 8) / 2^24, c0 = word 0 of Philox4x32-10, key (seed lo, seed hi), counter (step lo, step hi, row, 0x5A3C)
    token = the first i with cdf[i] > u * total; an entry without mass is never emitted

The kernel forms e, the sums and u * total in fp32, so a draw whose u * total lies within EPS * total of a boundary between two tokens may
fall on either side.  `accepted` is the set of tokens that leaves open, and the assertion used everywhere (judge / assert_draws) is:

    EVERY draw lies in its accepted set, and where that set has one member the draw is the reference's token, exactly.

EPS = 2^-17 is derived, not tuned:
    a term's exponential carries the fp32 rounding of its argument; the terms below x - max = -30 hold under 1e-13 of the mass, so this
        is at most 30 * 2^-24 relative                                                                              ~ 1.8e-6
    the fp32 sums add at most (chunk + 10 scan levels + 1) * 2^-24, at V = 50257 (chunk 50)                          ~ 3.6e-6
    u * total rounds once                                                                                            ~ 0.06e-6
    together ~ 5.5e-6 < 2^-17 ~ 7.6e-6.
It is never loosened to make a run pass: an excursion (the distance of u * total from the drawn token's interval in units of EPS * total)
above 1 is a finding about the kernel."""
import numpy as np

EPS = 2.0 ** -17
MIN_MARGIN = 0.02            # nucleus cases: every kept token's mass_gt / total lies at least this far from top_p (the header allows 1e-4)
SAMPLE_THREADS = 1024        # the block of sample_topk_kernel: thread t owns the indices [t * chunk, (t + 1) * chunk), chunk = ceil(V / 1024)
COUNTER_TAG = 0x5A3C         # word 3 of the sampler's Philox counter
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon et al., SC'11) on python ints: key (k0, k1), counter (c0, c1, c2, c3) -> 4 words"""
    k0, k1 = key
    c = list(ctr)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def counter_word(seed, step, row, tag=COUNTER_TAG):
    """word 0 of the sampler's Philox block for (seed, step, row): 64-bit seed and step as the device holds them, split into 32-bit halves"""
    seed, step = int(seed) & M64, int(step) & M64
    return philox4x32_10((seed & M32, seed >> 32), (step & M32, step >> 32, int(row) & M32, tag))[0]


def uniform(seed, step, row):
    """the kernel's u in [0, 1): the high 24 bits of the word, exact as a python float"""
    return (counter_word(seed, step, row) >> 8) / 16777216.0


def chunk_of(V):
    return -(-V // SAMPLE_THREADS)


def scaled(logits32, T):
    """x32 = logits * (1.0f / T), both in fp32 as the host wrapper and the kernel compute them"""
    logits32 = np.asarray(logits32)
    assert logits32.dtype == np.float32 and logits32.ndim == 1
    return logits32 * (np.float32(1.0) / np.float32(T))


def topk_rule(x, top_k):
    """bool [V]: x_i >= the k-th largest value, ties kept; top_k None / <= 0 / >= V: everything"""
    V = x.size
    if not top_k or top_k <= 0 or top_k >= V:
        return np.ones(V, bool)
    return x >= np.partition(x, V - top_k)[V - top_k]


def nucleus_rule(x, in_k, top_p):
    """Rules 2-4 of fk_sample_topp (include/franken_hip.h) on the scaled values x (float64 [V]) and the top-k set in_k:
    -> (kept bool [V], margin = min over in_k of |mass_gt / total - top_p|, e float64 [V]: exp(x - max in_k) on in_k, 0 elsewhere)"""
    e = np.zeros(x.size, np.float64)
    e[in_k] = np.exp(x[in_k] - x[in_k].max())
    total = e.sum()
    vals, inv = np.unique(x[in_k], return_inverse=True)                 # distinct kept values, ascending
    mass = np.bincount(inv.ravel(), weights=e[in_k], minlength=vals.size)
    gt = mass[::-1].cumsum()[::-1] - mass                               # value -> mass of the strictly larger ones
    mass_gt = np.full(x.size, np.inf)
    mass_gt[in_k] = gt[inv.ravel()]
    kept = in_k & (mass_gt < top_p * total)
    margin = float(np.abs(mass_gt[in_k] / total - top_p).min())
    return kept, margin, e


def nucleus_ref(logits, temperature, top_k, top_p):
    """logits fp32 [V], one row -> (kept bool [V], margin, probs float64 [V]: the distribution renormalised over the kept tokens)"""
    x = logits.astype(np.float64) / float(temperature)
    kept, margin, e = nucleus_rule(x, topk_rule(x, top_k), top_p)
    return kept, margin, np.where(kept, e, 0.0) / e[kept].sum()


class MarginError(AssertionError):
    """a nucleus row whose boundary lies too close to top_p for a reference to say which side a token falls on"""


def kept(logits32, T, top_k, top_p=1.0, min_margin=MIN_MARGIN):
    """bool [V]: the tokens the kernel draws from.  The top-k rule on the fp32 x (ties are the kernel's), then for top_p < 1 the nucleus rule,
    which needs a margin >= MIN_MARGIN: a condition on the inputs, asserted here (min_margin: for logits a test cannot shape, see
    tests/test_sample_draws_gpu.py)"""
    x32 = scaled(logits32, T)
    in_k = topk_rule(x32, top_k)
    if top_p is None or top_p >= 1.0:
        return in_k
    keep, margin, _ = nucleus_rule(x32.astype(np.float64), in_k, float(top_p))
    if margin < min_margin:
        raise MarginError(f"nucleus margin {margin:.2e} < {min_margin}: reshape the row")
    return keep


class RowRef:
    """One row's CDF in float64, index order.  Built from the scaled fp32 values and the kept mask, so that a defect test can hand in a
    wrong mask or wrong values; row_ref() builds the right one.  All queries take a scalar or an array of u."""

    def __init__(self, x32, keep):
        x = np.asarray(x32, np.float64)
        assert keep.any(), "no token kept"
        e = np.zeros(x.size, np.float64)
        with np.errstate(invalid="ignore"):
            e[keep] = np.exp(x[keep] - x[keep].max())
        self.V = x.size
        self.cdf = np.cumsum(e)
        self.total = float(self.cdf[-1])
        assert np.isfinite(self.total) and self.total >= 1.0, "a kept row holds its own maximum: total >= 1"
        self.npos = np.concatenate(([0], np.cumsum(e > 0.0))).astype(np.int32)      # npos[i]: entries with mass below index i

    def _prev(self, i):
        return np.where(i > 0, self.cdf[np.maximum(i - 1, 0)], 0.0)

    def has_mass(self, i):
        i = np.asarray(i)
        ok = (i >= 0) & (i < self.V)
        j = np.clip(i, 0, self.V - 1)
        return ok & (self.npos[j + 1] > self.npos[j])

    def probs(self):
        return np.diff(self.cdf, prepend=0.0) / self.total

    def want(self, u):
        """the first index whose cumulative mass exceeds u * total"""
        return np.searchsorted(self.cdf, np.asarray(u, np.float64) * self.total, side="right")

    def window(self, u):
        """(lo, hi): the indices i with cdf[i-1] - d <= t <= cdf[i] + d, d = EPS * total, are lo .. hi; those with mass are accepted"""
        t, d = np.asarray(u, np.float64) * self.total, EPS * self.total
        lo = np.searchsorted(self.cdf, t - d, side="left")
        hi = np.searchsorted(self.cdf, t + d, side="right")            # cdf[hi - 1] <= t + d < cdf[hi]: prev(hi) <= t + d
        return lo, np.minimum(hi, self.V - 1)

    def n_accepted(self, u):
        lo, hi = self.window(u)
        return self.npos[hi + 1] - self.npos[np.minimum(lo, self.V)]

    def accepted(self, u):
        lo, hi = self.window(float(u))
        i = np.arange(int(lo), int(hi) + 1)
        return i[self.has_mass(i)]

    def is_accepted(self, got, u):
        got = np.asarray(got)
        lo, hi = self.window(u)
        return (got >= lo) & (got <= hi) & self.has_mass(got)

    def excursion(self, got, u):
        """distance of t = u * total from got's interval [cdf[got-1], cdf[got]] in units of EPS * total: 0 inside, inf for an index that
        is outside the row or holds no mass"""
        got = np.asarray(got)
        t = np.asarray(u, np.float64) * self.total
        j = np.clip(got, 0, self.V - 1)
        dist = np.maximum(0.0, np.maximum(self._prev(j) - t, t - self.cdf[j])) / (EPS * self.total)
        return np.where(self.has_mass(got), dist, np.inf)


def row_ref(logits32, T, top_k, top_p=1.0, min_margin=MIN_MARGIN):
    return RowRef(scaled(logits32, T), kept(logits32, T, top_k, top_p, min_margin))


def draw(logits32, T, top_k, top_p, u):
    """-> (want, accepted, excursion): the reference's token for this u, every token the kernel's fp32 arithmetic may turn it into (an int
    array, ascending), and excursion(got) as RowRef.excursion"""
    r = row_ref(logits32, T, top_k, top_p)
    return int(r.want(u)), r.accepted(u), lambda got: float(r.excursion(got, u))


def judge(rows, us, got):
    """rows: RowRef per draw, us: its u, got: the token drawn.  -> (bad, n_ambiguous, largest excursion): bad lists every draw that breaks
    the rule as (draw number, got, want, accepted, excursion)"""
    bad, n_amb, worst = [], 0, 0.0
    for n, (r, u, g) in enumerate(zip(rows, us, got)):
        g = int(g)
        exc = float(r.excursion(g, u))
        worst = max(worst, exc)
        n_acc = int(r.n_accepted(u))
        n_amb += n_acc > 1
        want = int(r.want(u))
        if not bool(r.is_accepted(g, u)) or (n_acc == 1 and g != want):
            bad.append((n, g, want, r.accepted(u).tolist()[:8], exc))
    return bad, n_amb, worst


def assert_draws(rows, us, got, label=""):
    """the assertion used everywhere; -> the largest excursion (<= 1 when it passes)"""
    bad, _, worst = judge(rows, us, got)
    assert not bad, f"{label}: {len(bad)} of {len(us)} draws outside the accepted set (draw, got, want, accepted, excursion): {bad[:6]}"
    return worst
