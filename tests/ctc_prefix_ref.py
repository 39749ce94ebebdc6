"""Numpy restatement of the CTC prefix scorer of joint CTC / attention decoding (fk_ctc_prefix_init / fk_ctc_prefix_score; the rule is
stated in include/franken_hip.h).  Every function works in the dtype of the `y` it is given: np.float64 is the oracle, np.float32 the
same arithmetic at the kernels' precision, which the GPU tests use to size their tolerance.  The recursions run frame by frame in the
order of the rule and are vectorised over hypotheses only.  Nothing here imports the package."""
import itertools

import numpy as np

FLOOR = -1e10
NONE, BAD = -1, -2


def log_softmax_rows(logits, dtype=np.float64):
    """y [T, C] = logits - row logsumexp, in `dtype` (the max is subtracted first)"""
    x = np.asarray(logits).astype(dtype)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype)))


def lae(a, b):
    with np.errstate(invalid="ignore"):
        return np.logaddexp(a, b)


class Hyps:
    """the states of n hypotheses of one sentence: r_n / r_b [n, Tg], psi [n], last int [n]"""

    def __init__(self, r_n, r_b, psi, last):
        self.r_n, self.r_b, self.psi, self.last = r_n, r_b, psi, np.asarray(last, np.int64)

    def __len__(self):
        return len(self.psi)

    def take(self, idx):
        idx = np.atleast_1d(np.asarray(idx, np.int64))
        return Hyps(self.r_n[idx].copy(), self.r_b[idx].copy(), self.psi[idx].copy(), self.last[idx].copy())

    @staticmethod
    def cat(parts):
        return Hyps(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("r_n", "r_b", "psi", "last")))


def empty(y, blank, n=1):
    """n copies of the empty hypothesis; y [Tg, C] is already cut to the sentence's frames; r_b is summed in frame order"""
    dt = y.dtype
    r_b = np.empty(len(y), dt)
    acc = dt.type(0)
    for t in range(len(y)):
        acc = dt.type(acc + y[t, blank])
        r_b[t] = acc
    return Hyps(np.full((n, len(y)), -np.inf, dt), np.tile(r_b, (n, 1)), np.zeros(n, dt), np.full(n, NONE))


def _valid(cs, C, blank):
    return (cs >= 0) & (cs < C) & (cs != blank)


def extend(y, blank, h, cs, states=True):
    """hypothesis i of h extended by label cs[i] -> Hyps (states=False: only psi is computed, r_n / r_b are None).  A label outside
    [0, C) or equal to the blank gives the impossible hypothesis: everything -inf, last = BAD."""
    dt = y.dtype
    Tg, C = y.shape
    cs = np.asarray(cs, np.int64)
    n = len(cs)
    ok = _valid(cs, C, blank)
    col = np.where(ok, cs, 0)
    ninf = dt.type(-np.inf)
    N, B = (np.full((n, Tg), ninf, dt), np.full((n, Tg), ninf, dt)) if states else (None, None)
    psi = np.full(n, ninf, dt)
    if Tg > 0:
        n_prev = np.where(ok & (h.last == NONE), y[0, col], ninf).astype(dt)
        b_prev = np.full(n, ninf, dt)
        psi = n_prev.copy()
        same = cs == h.last
        if states:
            N[:, 0] = n_prev
        for t in range(1, Tg):
            yt = np.where(ok, y[t, col], ninf).astype(dt)
            phi = np.where(same, h.r_b[:, t - 1], lae(h.r_n[:, t - 1], h.r_b[:, t - 1]))
            psi = lae(psi, phi + yt)
            if states:
                n_new = lae(n_prev, phi) + yt
                b_prev = lae(n_prev, b_prev) + y[t, blank]
                n_prev = n_new
                N[:, t], B[:, t] = n_prev, b_prev
    return Hyps(N, B, psi, np.where(ok, cs, BAD))


def full(h):
    """log-probability of the whole labelling: lae(r_n[Tg-1], r_b[Tg-1]); -inf without a frame"""
    if h.r_n.shape[1] == 0:
        return np.full(len(h), -np.inf, h.r_n.dtype)
    return lae(h.r_n[:, -1], h.r_b[:, -1])


def delta(y, blank, h, cs, eos=-1):
    """the candidate terms of hypothesis i for label cs[i]: psi(h c) - psi(h), the whole-labelling term for c == eos, FLOOR where the
    rule says so"""
    dt = y.dtype
    Tg, C = y.shape
    cs = np.asarray(cs, np.int64)
    if Tg == 0:
        return np.full(len(cs), FLOOR, dt)
    is_eos = (cs == eos) & (eos >= 0)
    p2 = np.where(is_eos, full(h), extend(y, blank, h, np.where(is_eos, -1, cs), states=False).psi)
    with np.errstate(invalid="ignore"):
        d = (p2 - h.psi).astype(dt)
    return np.where(np.isfinite(p2) & np.isfinite(h.psi), d, dt.type(FLOOR)).astype(dt)


def joint(lp, d, weight, dtype):
    """(1 - weight) * lp + weight * delta in this order, every operation rounded to `dtype` (fp32: the kernel's subtraction, two
    multiplies and one add); the weight is the fp32 value the kernel is handed"""
    lp, d = np.asarray(lp).astype(dtype), np.asarray(d).astype(dtype)
    t = np.dtype(dtype).type
    w = t(np.float32(weight))
    return ((t(1) - w) * lp + w * d).astype(dtype)


def score_rows(ys, blank, hyps, top_lp, top_id, weight, eos=-1, fin=None, W=1, broadcast=False):
    """The scoring half of one fk_ctc_prefix_score launch.  ys: the sentences' y [Tg, C] (their dtype is the dtype of the arithmetic);
    hyps: one Hyps of W rows per sentence; top_lp / top_id [rows, k], rows = S * W or S (broadcast: the sentence's row 0 scores).
    -> (joint [rows, k], floor mask [rows, k]); rows of finished beams keep top_lp and are not floor entries."""
    rows, k = top_lp.shape
    dt = ys[0].dtype
    out = np.asarray(top_lp).astype(dt).copy()
    floor = np.zeros((rows, k), bool)
    for q in range(rows):
        g, b = (q, 0) if broadcast else divmod(q, W)
        if fin is not None and fin[g * W + b]:
            continue
        d = delta(ys[g], blank, hyps[g].take(np.full(k, b)), top_id[q], eos)
        floor[q] = d == dt.type(FLOOR)
        out[q] = joint(top_lp[q], d, weight, dt)
    return out, floor


def brute_prefix(y, blank, prefix, whole=False):
    """log of the summed probability of every path of C^T whose collapsed labelling starts with (whole: equals) `prefix`; float64"""
    T, C = y.shape
    tot = -np.inf
    for path in itertools.product(range(C), repeat=T):
        lab = [k for k, _ in itertools.groupby(path) if k != blank]
        if (lab == list(prefix)) if whole else (lab[:len(prefix)] == list(prefix)):
            tot = np.logaddexp(tot, sum(y[t, c] for t, c in enumerate(path)))
    return tot


def hyp_of(y, blank, labels):
    """the one hypothesis `labels` (a list), from the empty one"""
    h = empty(y, blank)
    for c in labels:
        h = extend(y, blank, h, [c])
    return h
