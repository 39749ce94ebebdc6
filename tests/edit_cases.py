"""The cases tests/test_edit_cpu.py and tests/test_edit_gpu.py share, each with its result from tests/edit_ref.py (computed once, cached:
treat everything as read-only).

DISTANCE cases: every route of fk_edit_distance_route at its smallest and largest length and one past each lane boundary, with the
sequence of the narrower array on either side, n_a = n and n_a = 1, lengths given or marked by the pad value, clamped lengths, a
2-symbol alphabet (many ties in the table: every branch of the min), ids near +-2^62 that differ only above bit 32, identical sequences and
disjoint alphabets.  The sequences live in a larger buffer: behind every length and between the rows there is garbage that holds tokens of
the alphabet and look-alikes of the pad value, so a kernel that reads one entry too many gets another distance.

RANKING cases (pairwise distances + MBR): lists of edits of a common base sentence with scores N(-10, 3), best first.  make_ranking()
asserts that the smallest non-zero gap between two risks of a sentence is at least 16 * e32 (e32: the largest difference between the
float32 and the float64 run of the restatement), the rule of tests/rescore_cases.py; the seeds were picked on the CPU so that it holds.

MWER cases: logits, targets and a hypothesis list (passed to engine.ctc_mwer_loss through hyps=)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from tests import edit_ref as ER

PAD = -100
MARGIN = 16.0
FLOOR = 8.0 * 2.0 ** -24
BIG = [1 << 62, (1 << 62) + (1 << 33), -(1 << 62), -(1 << 62) + (1 << 40)]     # equal in their low 32 bits

#              La,   Lb,  lengths of a (per group),      lengths of b (per pair of a group),  n_a = 1, alphabet
DISTANCE = {
    "lane":       (64,   65,   [0, 1, 2, 63, 64],             [0, 1, 2, 63, 64, 65],            False, "four"),
    "lane_ref":   (64,   65,   [0, 1, 2, 63, 64],             [0, 1, 2, 63, 64, 65],            True,  "two"),
    "lane_swap":  (129,  64,   [0, 1, 65, 129],               [0, 2, 63, 64],                   False, "two"),    # b is the narrower array
    "lane_long":  (3,    1024, [0, 3],                        [1024, 255],                      True,  "four"),   # a short reference, long rows
    "rows4":      (256,  256,  [65, 127, 128, 129, 255, 256], [0, 1, 64, 65, 255, 256],         True,  "four"),
    "rows4_swap": (300,  65,   [129, 300],                    [65, 2],                          False, "two"),    # the route's smallest width
    "rows16_min": (257,  257,  [257],                         [257, 1],                         True,  "two"),
    "rows16":     (1024, 1024, [1024, 257],                   [1024, 300],                      False, "four"),
    "big_ids":    (8,    9,    [8, 5],                        [9, 8, 3],                        False, "big"),
    "same":       (64,   64,   [64, 17],                      [64, 17],                         False, "same"),
    "disjoint":   (20,   33,   [20, 5],                       [33, 7],                          False, "disjoint"),
    "clamp":      (8,    9,    [0, 8],                        [9, 0, 4],                        True,  "four"),   # lengths beyond the row / negative
}


def _tokens(rng, kind, side, k):
    if kind == "two":
        return [int(t) for t in rng.integers(1, 3, size=k)]
    if kind == "big":
        return [BIG[int(t)] for t in rng.integers(0, 4, size=k)]
    if kind == "disjoint":
        return [int(t) for t in rng.integers(1, 3, size=k) + (0 if side == "a" else 2)]
    return [int(t) for t in rng.integers(1, 5, size=k)]


def _garbage(rng, kind, shape):
    """what lies behind the lengths and between the rows: tokens of the alphabet and look-alikes of the pad value"""
    pool = np.array((BIG if kind == "big" else [1, 2, 3, 4]) + [PAD, PAD], dtype=np.int64)
    return pool[rng.integers(0, len(pool), size=shape)]


@functools.lru_cache(maxsize=None)
def make_distance(name, explicit):
    """-> SimpleNamespace(a int64 [B, n_a, La] and b int64 [B, n, Lb] (strided views into garbage), alen / blen int64 or None (explicit
    False: a sequence ends at its first PAD), dist int64 [B, n], alen_ref int64 [B, n_a], route)"""
    La, Lb, LA, LB, share, kind = DISTANCE[name]
    rng = np.random.default_rng(1000 + sorted(DISTANCE).index(name))
    B, n = len(LA), len(LB)
    n_a = 1 if share else n
    sa = _garbage(rng, kind, (B, n_a + 1, La + 3))
    sb = _garbage(rng, kind, (B, n + 1, Lb + 3))
    alen = np.zeros((B, n_a), dtype=np.int64)
    blen = np.zeros((B, n), dtype=np.int64)
    for g in range(B):
        for h in range(n):
            y = _tokens(rng, kind, "b", LB[h])
            if h < n_a:
                x = _tokens(rng, kind, "a", LA[g])
                if kind == "same":
                    x, y = (y[:LA[g]] + x)[:LA[g]], y
                sa[g, h, :len(x)] = x
                alen[g, h] = len(x)
                if not explicit and len(x) < La:
                    sa[g, h, len(x)] = PAD
            sb[g, h, :len(y)] = y
            blen[g, h] = len(y)
            if not explicit and len(y) < Lb:
                sb[g, h, len(y)] = PAD
    a, b = sa[:, :n_a, :La], sb[:, :n, :Lb]
    dist, alen_ref = ER.distances(a.tolist(), alen if explicit else None, b.tolist(), blen if explicit else None, PAD)
    if name == "clamp":                                                 # the same sequences under lengths outside [0, L]
        assert explicit
        alen, blen = np.where(alen == La, La + 5, -3), np.where(blen == Lb, Lb + 7, np.where(blen == 0, -1, blen))
    if kind == "same":
        assert all(dist[g, h] == 0 for g in range(B) for h in range(n) if LA[g] == LB[h])
    if kind == "disjoint":
        assert all(dist[g, h] == max(LA[g], LB[h]) for g in range(B) for h in range(n))
    t = torch.from_numpy
    return SimpleNamespace(a=t(sa)[:, :n_a, :La], b=t(sb)[:, :n, :Lb], alen=t(alen) if explicit else None, blen=t(blen) if explicit else None,
                           dist=dist, alen_ref=alen_ref, La=La, Lb=Lb, n=n, n_a=n_a)


#            B,  n,  T,   vocabulary, scale, seed
RANKING = {
    "r8":      (4,  8,  12,  6,  1.0, 1),
    "r32":     (3,  32, 25,  50, 0.5, 1),
    "r5":      (2,  5,  70,  41, 1.0, 1),       # T > 64: four rows per lane
    "r16":     (2,  16, 130, 41, 0.3, 1),
    "r3long":  (1,  3,  300, 41, 1.0, 1),       # T > 256: sixteen rows per lane
    "one":     (2,  1,  6,   6,  1.0, 1),       # n = 1: nothing to rank
    "invalid": (3,  8,  12,  6,  1.0, 1),       # some hypotheses invalid, then a sentence with all of them
    "ties":    (2,  8,  12,  6,  1.0, 1),       # duplicates with equal scores: exact ties, the smaller index wins
    "uniform": (2,  8,  12,  6,  0.0, 1),       # scale = 0: the uniform posterior (p = 1 / 8 exactly)
    "sharp":   (2,  8,  12,  6,  1e4, 1),       # every weight but the first is exactly 0: risk_i = dist[i][0], place 0 stays
    "outlier": (1,  6,  12,  20, 1.0, 1),       # the best-scored hypothesis is far from all others: MBR demotes it
}
GARBAGE = -(1 << 40)


def _edit(rng, s, V, k):
    s = list(s)
    for _ in range(k):
        kind, pos = rng.integers(3), int(rng.integers(len(s)))
        if kind == 0:
            s[pos] = int(rng.integers(V))
        elif kind == 1 and len(s) > 1:
            del s[pos]
        else:
            s.insert(pos, int(rng.integers(V)))
    return s


def generate_ranking(name):
    B, n, T, V, scale, seed = RANKING[name]
    rng = np.random.default_rng(7000 + 13 * sorted(RANKING).index(name) + seed)
    store = np.full((B, n + 1, T + 3), GARBAGE, dtype=np.int64)
    lengths = np.zeros((B, n), dtype=np.int64)
    scores = np.zeros((B, n), dtype=np.float32)
    for b in range(B):
        base = [int(t) for t in rng.integers(0, V, size=max(1, T - 2))]
        hyps = [base] + [_edit(rng, base, V, int(rng.integers(1, 4))) for _ in range(n - 1)]
        sc = np.sort(rng.normal(-10.0, 3.0, size=n).astype(np.float32))[::-1].copy()
        if name == "ties":
            hyps[4] = list(hyps[1]); sc[4] = sc[1] = sc[2]              # a duplicate, equal scores (and a third hypothesis at that score)
            hyps[6] = list(hyps[0])                                     # a duplicate with another score
        if name == "sharp":
            sc[1:] -= 0.5
            hyps = [h if i == 0 or h != hyps[0] else h + [0] for i, h in enumerate(hyps)]
        if name == "outlier":
            hyps[0] = [int(t) for t in rng.integers(V // 2, V, size=T)]
            hyps[1:] = [_edit(rng, [int(t) % (V // 2) for t in base], V // 2, 1) for _ in range(n - 1)]
            sc[0] = sc[1] + 0.5
        if name == "invalid":
            if b == 0:
                sc[2] = sc[5] = -np.inf; hyps[2] = []
            if b == 1:
                sc[:] = -np.inf
            if b == 2:
                sc[0] = np.nan                                          # not finite either
        hyps = [h[:T] for h in hyps]
        for h, s in enumerate(hyps):
            store[b, h, :len(s)] = s
            lengths[b, h] = len(s)
        scores[b] = sc
    t = torch.from_numpy
    return SimpleNamespace(ids=t(store)[:, :n, :T], lengths=t(lengths), scores=t(scores))


@functools.lru_cache(maxsize=None)
def make_ranking(name):
    """-> dict(inp, dist int64 [B, n, n], risk float64 [B, n], order int64 [B, n], n_valid [B], e32, gap, tol [B, n], scale)"""
    B, n, T, V, scale, _ = RANKING[name]
    inp = generate_ranking(name)
    ids, lengths, scores = inp.ids.numpy(), inp.lengths.numpy(), inp.scores.numpy()
    dist = np.zeros((B, n, n), dtype=np.int64)
    risk = np.zeros((B, n))
    order = np.zeros((B, n), dtype=np.int64)
    n_valid = np.zeros(B, dtype=np.int64)
    e32, gap = 0.0, np.inf
    for b in range(B):
        dist[b] = ER.pairwise(ids[b].tolist(), lengths[b], scores[b])
        risk[b], order[b], n_valid[b] = ER.mbr(dist[b], scores[b], scale)
        r32, o32, _ = ER.mbr(dist[b], scores[b], scale, np.float32)
        ok = np.isfinite(scores[b])
        if ok.any():
            e32 = max(e32, float(np.abs(r32[ok].astype(np.float64) - risk[b][ok]).max()))
        gap = min(gap, ER.smallest_gap(risk[b], ok))
    assert gap >= MARGIN * e32, (name, gap, e32)
    if name == "outlier":
        assert order[0, 0] != 0
    if name == "sharp":
        assert np.all(order[:, 0] == 0)
    if name == "ties":
        assert list(order[0]).index(1) < list(order[0]).index(4)
    tol = np.maximum(4.0 * e32, FLOOR * np.maximum(1.0, np.abs(np.where(np.isfinite(risk), risk, 0.0))))
    return dict(name=name, inp=inp, dist=dist, risk=risk, order=order, n_valid=n_valid, e32=e32, gap=gap, tol=tol, scale=scale, B=B, n=n, T=T)


#          B, T,  C,  columns of the hypothesis array (> 31: the LDS route of the CTC kernels), seed
MWER = {
    "small": (3, 12, 5,  8,  1),
    "lds":   (2, 70, 41, 40, 2),
}


@functools.lru_cache(maxsize=None)
def make_mwer(name, nbest):
    """-> SimpleNamespace(logits fp32 [B, T, C], targets int64 [B, 4] padded with PAD, target_lengths [B], ids [B, nbest, Th], lengths,
    scores): 2 to 3 labels per target, blank 0; hypothesis 0 is the target, the others are edits of it.  With nbest = 4: an empty beam slot,
    an infeasible labelling (8 equal labels in 12 frames) with a finite score, and a last sentence whose hypotheses are all invalid."""
    B, T, C, Th, seed = MWER[name]
    rng = np.random.default_rng(8100 + seed)
    g = torch.Generator().manual_seed(8200 + seed)
    logits = 1.5 * torch.randn((B, T, C), generator=g)
    targets = np.full((B, 4), PAD, dtype=np.int64)
    tlen = np.zeros(B, dtype=np.int64)
    ids = np.full((B, nbest, Th), PAD, dtype=np.int64)
    lengths = np.zeros((B, nbest), dtype=np.int64)
    scores = np.zeros((B, nbest), dtype=np.float32)
    for b in range(B):
        k = 2 + b % 2
        tg = [int(t) for t in rng.integers(1, C, size=k)]
        targets[b, :k], tlen[b] = tg, k
        hyps = [tg] + [[1 + t for t in _edit(rng, [t - 1 for t in tg], C - 1, 1 + i % 2)][:4] for i in range(nbest - 1)]
        sc = np.sort(rng.normal(-6.0, 2.0, size=nbest).astype(np.float32))[::-1].copy()
        if nbest == 4:
            if b == 0:
                hyps[3], sc[3] = [], -np.inf                            # the beam search's empty slot
            if b == 1 and name == "small":
                hyps[2] = [2] * 8                                       # needs 15 frames: nll = inf
        if b == B - 1 and name == "small":
            sc[:] = -np.inf
        for i, h in enumerate(hyps):
            ids[b, i, :len(h)] = h
            lengths[b, i] = len(h)
        scores[b] = sc
    t = torch.from_numpy
    return SimpleNamespace(logits=logits, targets=t(targets), target_lengths=t(tlen), ids=t(ids), lengths=t(lengths), scores=t(scores), blank=0)
