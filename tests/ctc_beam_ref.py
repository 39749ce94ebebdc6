"""Numpy restatement of the CTC prefix beam search (fk_ctc_beam_search, csrc/ctc.hip) as the plain dictionary algorithm.

A beam is a set of prefixes (tuples of non-blank labels), each with (pb, pnb): the log-mass of the alignments of the frames so far that
end in blank / in the prefix's last label; total = logaddexp(pb, pnb).  It starts as {(): (0, -inf)}.  Per frame t < T_b:
  lp          log_softmax of the row, in `dtype`
  candidates  the min(K, C - 1) non-blank classes with the largest RAW logit, equal logits by ascending class id (exact compares: the
              set is the same in float32 and float64)
  every prefix p of the beam, last label e:
      p          pb'  += total + lp[blank]
      p          pnb' += pnb + lp[e]                                 (p non-empty; whether or not e is a candidate)
      p + (c,)   pnb' += (pb if c == e else total) + lp[c]           for every c that is a candidate OR for which p + (c,) is in the beam
  the W entries of the new table with the largest total survive; an entry whose total is -inf never does.
Pruning limits which NEW prefixes are proposed, never the flow of probability between prefixes that are already in the beam.

Exact ties follow the kernel's fixed order: a resident prefix before a new one, then the lower position in the beam (of the prefix, or of
a new prefix's parent; the beam is kept in the order of the last selection), then the better candidate.  Such ties are real: two
candidates with equal logits behind one parent are the same sum of the same addends in every arithmetic (bf16-rounded logits produce
them all the time).  The gaps this file reports leave them out and list where they occurred instead.

`dtype` is the arithmetic of lp and of every logaddexp: float64 is the yardstick, float32 the measure of what fp32 arithmetic costs."""
import numpy as np


def _lae(a, b):
    """logaddexp in the arguments' own dtype; (-inf, -inf) -> -inf without a warning"""
    with np.errstate(invalid="ignore"):
        return np.logaddexp(a, b)


def candidates(row, blank, K):
    """ids of the min(K, C - 1) non-blank classes with the largest raw value, descending, equal values by ascending id"""
    ids = np.delete(np.arange(len(row), dtype=np.int64), blank)
    vals = row[ids].astype(np.float64)
    if len(ids) > K:                                               # only what reaches the K-th largest value takes part in the sort
        keep = vals >= np.partition(vals, len(ids) - K)[len(ids) - K]
        ids, vals = ids[keep], vals[keep]
    order = np.lexsort((ids, -vals))                               # the last key is the primary one
    return [int(c) for c in ids[order[:K]]]


def search_one(x, blank, W, K, dtype=np.float64):
    """x [T_b, C] raw logits of one sample -> (hyps, frame_gap, ties): hyps = the final beam [(prefix, total)] by total descending;
    frame_gap = the smallest non-zero total[W - 1] - total[W] of the sorted new table over all frames (inf when there is none);
    ties = the places where that difference, or the difference of two neighbouring final totals, is exactly 0: ("frame", t) /
    ("final", i)."""
    dt = np.dtype(dtype).type
    NEG = dt(-np.inf)
    beam = [((), dt(0.0), NEG)]                                    # in the order of the last selection
    frame_gap, ties = np.inf, []
    for t in range(x.shape[0]):
        raw = x[t]
        row = raw.astype(dtype)
        m = row.max()
        lp = row - (m + np.log(np.exp(row - m).sum(dtype=dtype)))
        cand = candidates(raw, blank, K)
        rank = {c: k for k, c in enumerate(cand)}
        where = {p: j for j, (p, _, _) in enumerate(beam)}
        kids = {}                                                  # prefix -> the labels c for which prefix + (c,) is in the beam
        for q in where:
            if q:
                kids.setdefault(q[:-1], []).append(q[-1])
        new = {}                                                   # prefix -> [pb, pnb, place in the order of exact ties]

        def add(p, pb, pnb, place):
            o = new.get(p)
            if o is None:
                new[p] = [pb, pnb, place]
            else:
                o[0], o[1] = _lae(o[0], pb), _lae(o[1], pnb)

        for j, (p, pb, pnb) in enumerate(beam):
            tot = _lae(pb, pnb)
            add(p, tot + lp[blank], NEG, j)
            e = p[-1] if p else None
            if p:
                add(p, NEG, pnb + lp[e], j)
            for c in cand + [c for c in kids.get(p, ()) if c not in rank]:
                q = p + (c,)
                add(q, NEG, (pb if c == e else tot) + lp[c], where[q] if q in where else W + j * len(cand) + rank[c])
        table = [(p, v[0], v[1], _lae(v[0], v[1]), v[2]) for p, v in new.items()]
        table = [r for r in table if r[3] > NEG]
        table.sort(key=lambda r: (-float(r[3]), r[4]))
        if len(table) > W:
            gap = float(table[W - 1][3]) - float(table[W][3])
            if gap == 0.0:
                ties.append(("frame", t))
            else:
                frame_gap = min(frame_gap, gap)
        beam = [(p, pb, pnb) for p, pb, pnb, _, _ in table[:W]]
    hyps = [(p, float(_lae(pb, pnb))) for p, pb, pnb in beam]
    ties += [("final", i) for i in range(len(hyps) - 1) if hyps[i][1] == hyps[i + 1][1]]
    return hyps, frame_gap, ties


def beam_search(logits, input_lengths=None, blank=0, beam_width=8, topk=None, nbest=1, pad=-100, dtype=np.float64):
    """logits [B, T, C] -> dict: ids int64 [B, nbest, T] padded with `pad`, lengths int64 [B, nbest], scores float64 [B, nbest] (-inf and
    length 0 for a slot without hypothesis), hyps (per sample the whole final beam), frame_gap [B], final_gap [B] (the smallest non-zero
    difference between neighbouring totals of the final beam; inf without one) and ties (per sample, see search_one)."""
    x = np.asarray(logits)
    B, T, C = x.shape
    K = min(32, C - 1) if topk is None else min(int(topk), C - 1)
    ids = np.full((B, nbest, T), pad, dtype=np.int64)
    lengths = np.zeros((B, nbest), dtype=np.int64)
    scores = np.full((B, nbest), -np.inf)
    hyps_all, ties_all, frame_gap, final_gap = [], [], np.full(B, np.inf), np.full(B, np.inf)
    for b in range(B):
        tb = T if input_lengths is None else min(max(int(input_lengths[b]), 0), T)
        hyps, frame_gap[b], ties = search_one(x[b, :tb], blank, beam_width, K, dtype)
        hyps_all.append(hyps)
        ties_all.append(ties)
        tot = [s for _, s in hyps]
        final_gap[b] = min([tot[i] - tot[i + 1] for i in range(len(tot) - 1) if tot[i] != tot[i + 1]], default=np.inf)
        for h, (p, s) in enumerate(hyps[:nbest]):
            ids[b, h, :len(p)] = p
            lengths[b, h] = len(p)
            scores[b, h] = s
    return dict(ids=ids, lengths=lengths, scores=scores, hyps=hyps_all, ties=ties_all, frame_gap=frame_gap, final_gap=final_gap)


def brute_force(x, blank):
    """x [T, C] -> {labelling: log-probability}: all C^T alignments in float64, grouped by their collapsed labelling"""
    import itertools
    x = np.asarray(x, dtype=np.float64)
    T, C = x.shape
    m = x.max(axis=1, keepdims=True)
    lp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    out = {}
    for path in itertools.product(range(C), repeat=T):
        s = sum(lp[t, c] for t, c in enumerate(path))
        lab = tuple(c for t, c in enumerate(path) if c != blank and (t == 0 or c != path[t - 1]))
        out[lab] = np.logaddexp(out[lab], s) if lab in out else s
    return out
