"""Numpy restatement of the CTC prefix beam search with n-gram shallow fusion (fk_ctc_beam_search_lm, csrc/ctc.hip): the dictionary
algorithm of tests/ctc_beam_ref.py with another selection key.

The acoustic recursion is ctc_beam_ref's, statement by statement.  A prefix also carries
    lmw(p + (c,)) = lmw(p) + (lm_weight * ln P_lm(c | p) + length_bonus),   lm(p + (c,)) = lm(p) + ln P_lm(c | p),   lmw(()) = lm(()) = 0
and the W entries with the largest key = total + lmw survive; an entry whose total is -inf never does; exact ties keep ctc_beam_ref's
order.  With use_eos the final beam is sorted once more by key + lm_weight * ln P_lm(</s> | p) (stable: equal keys in the order of the last
selection) and lm includes that term.  ln P_lm is NGramLM.score, the plain recursive backoff definition in float64 straight from the
model's dicts (never the compiled tables), under the context model.start_context + p.

`dtype` is the arithmetic of lp, of every logaddexp AND of the lmw / lm sums and the keys (the float64 score is rounded to `dtype`
first): float64 is the yardstick, the float32 run measures everything fp32 costs.  frame_gap, final_gap and ties are those of
ctc_beam_ref, on the fused keys."""
import numpy as np

from tests.ctc_beam_ref import _lae, candidates


def search_one(x, lm, blank, W, K, lm_weight=1.0, length_bonus=0.0, use_eos=True, dtype=np.float64, stats=None):
    """x [T_b, C] raw logits of one sample -> (hyps, frame_gap, ties): hyps = the final beam [(prefix, am, lm, total)] best first;
    frame_gap = the smallest non-zero key[W - 1] - key[W] of the sorted new table over all frames (inf when there is none); ties = the
    places where that difference, or the difference of two neighbouring final keys, is exactly 0: ("frame", t) / ("final", i).
    stats (a dict): counts look-ups by the number of backoff levels they took ("levels": list) and records every beam ("beams")."""
    dt = np.dtype(dtype).type
    NEG = dt(-np.inf)
    w, bonus = dt(lm_weight), dt(length_bonus)
    start = tuple(lm.start_context)
    beam = [((), dt(0.0), NEG, dt(0.0), dt(0.0))]                  # (prefix, pb, pnb, lmw, lm) in the order of the last selection
    frame_gap, ties = np.inf, []
    for t in range(x.shape[0]):
        raw = x[t]
        row = raw.astype(dtype)
        m = row.max()
        lp = row - (m + np.log(np.exp(row - m).sum(dtype=dtype)))
        cand = candidates(raw, blank, K)
        rank = {c: k for k, c in enumerate(cand)}
        where = {p: j for j, (p, _, _, _, _) in enumerate(beam)}
        kids = {}
        for q in where:
            if q:
                kids.setdefault(q[:-1], []).append(q[-1])
        new = {}                                                   # prefix -> [pb, pnb, place in the order of exact ties, lmw, lm]

        def add(p, pb, pnb, place, lmw, lms):
            o = new.get(p)
            if o is None:
                new[p] = [pb, pnb, place, lmw, lms]
            else:
                o[0], o[1] = _lae(o[0], pb), _lae(o[1], pnb)

        for j, (p, pb, pnb, lmw, lms) in enumerate(beam):
            tot = _lae(pb, pnb)
            add(p, tot + lp[blank], NEG, j, lmw, lms)
            e = p[-1] if p else None
            if p:
                add(p, NEG, pnb + lp[e], j, lmw, lms)
            for c in cand + [c for c in kids.get(p, ()) if c not in rank]:
                q = p + (c,)
                if q in where:                                     # a resident prefix carries its own term
                    add(q, NEG, (pb if c == e else tot) + lp[c], where[q], beam[where[q]][3], beam[where[q]][4])
                else:
                    s = dt(lm.score(start + p, c))
                    if stats is not None:
                        stats.setdefault("levels", []).append(_levels(lm, start + p, c))
                    add(q, NEG, (pb if c == e else tot) + lp[c], W + j * len(cand) + rank[c], lmw + (w * s + bonus), lms + s)
        table = [(p, v[0], v[1], _lae(v[0], v[1]), v[2], v[3], v[4]) for p, v in new.items()]
        table = [r + (r[3] + r[5],) for r in table if r[3] > NEG]
        table = [r for r in table if r[7] > NEG]
        table.sort(key=lambda r: (-float(r[7]), r[4]))
        if len(table) > W:
            gap = float(table[W - 1][7]) - float(table[W][7])
            if gap == 0.0:
                ties.append(("frame", t))
            else:
                frame_gap = min(frame_gap, gap)
        beam = [(p, pb, pnb, lmw, lms) for p, pb, pnb, _, _, lmw, lms, _ in table[:W]]
        if stats is not None:
            stats.setdefault("beams", []).append([p for p, _, _, _, _ in beam])
    final = []
    for p, pb, pnb, lmw, lms in beam:
        am = _lae(pb, pnb)
        key = am + lmw
        if use_eos:
            s = dt(lm.score(start + p, lm.eos))
            key, lms = key + w * s, lms + s
        final.append((p, float(am), float(lms), float(key)))
    final.sort(key=lambda r: -r[3])                                # stable
    ties += [("final", i) for i in range(len(final) - 1) if final[i][3] == final[i + 1][3]]
    return final, frame_gap, ties


def _levels(lm, ctx, c):
    """how many times the backoff definition shortens the context (truncated to order - 1) before (context, c) is listed"""
    ctx = tuple(ctx)[-(lm.order - 1):] if lm.order > 1 else ()
    n = 0
    while ctx + (c,) not in lm.ngrams:
        ctx, n = ctx[1:], n + 1
    return n


def beam_search(logits, lm, input_lengths=None, blank=0, beam_width=8, topk=None, nbest=1, lm_weight=1.0, length_bonus=0.0, use_eos=True,
                pad=-100, dtype=np.float64, stats=None):
    """logits [B, T, C] -> dict: ids int64 [B, nbest, T] padded with `pad`, lengths int64 [B, nbest], am / lm / total float64 [B, nbest]
    (-inf and length 0 for a slot without hypothesis), hyps (per sample the whole final beam), frame_gap [B], final_gap [B] (the smallest
    non-zero difference between neighbouring final keys; inf without one) and ties (per sample, see search_one)."""
    x = np.asarray(logits)
    B, T, C = x.shape
    K = min(32, C - 1) if topk is None else min(int(topk), C - 1)
    ids = np.full((B, nbest, T), pad, dtype=np.int64)
    lengths = np.zeros((B, nbest), dtype=np.int64)
    am, lms, total = (np.full((B, nbest), -np.inf) for _ in range(3))
    hyps_all, ties_all, frame_gap, final_gap = [], [], np.full(B, np.inf), np.full(B, np.inf)
    for b in range(B):
        tb = T if input_lengths is None else min(max(int(input_lengths[b]), 0), T)
        st = None if stats is None else stats.setdefault(b, {})
        hyps, frame_gap[b], ties = search_one(x[b, :tb], lm, blank, beam_width, K, lm_weight, length_bonus, use_eos, dtype, st)
        hyps_all.append(hyps)
        ties_all.append(ties)
        key = [r[3] for r in hyps]
        final_gap[b] = min([key[i] - key[i + 1] for i in range(len(key) - 1) if key[i] != key[i + 1]], default=np.inf)
        for h, (p, a, l, k) in enumerate(hyps[:nbest]):
            ids[b, h, :len(p)] = p
            lengths[b, h] = len(p)
            am[b, h], lms[b, h], total[b, h] = a, l, k
    return dict(ids=ids, lengths=lengths, am=am, lm=lms, total=total, hyps=hyps_all, ties=ties_all, frame_gap=frame_gap, final_gap=final_gap)


def brute_force(x, lm, blank, lm_weight=1.0, length_bonus=0.0, use_eos=True):
    """x [T, C] -> {labelling: (am, lm, total)} over all C^T alignments in float64: total = am + lm_weight * lm + length_bonus * len"""
    from tests.ctc_beam_ref import brute_force as am_brute_force
    start = tuple(lm.start_context)
    out = {}
    for p, am in am_brute_force(x, blank).items():
        s = sum(lm.score(start + p[:i], c) for i, c in enumerate(p))
        if use_eos:
            s += lm.score(start + p, lm.eos)
        out[p] = (am, s, am + lm_weight * s + length_bonus * len(p))
    return out
