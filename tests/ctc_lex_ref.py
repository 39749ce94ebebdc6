"""Numpy restatement of the lexicon-constrained CTC prefix beam search (fk_ctc_beam_search_lex, csrc/ctc.hip): the dictionary algorithm
of tests/ctc_beam_ref.py, with the lexicon as a plain dict {pronunciation: [word ids, ascending]} plus the set of its prefixes, and the
word model scored through NGramLM.score, the dictionary definition.  No hash table and no trie.

The acoustic recursion is ctc_beam_ref's, statement by statement, over labellings of the head's classes, `sep` included.  A prefix also
carries `part` (the pronunciation of its unfinished word, () at a word start), `words` (the words it closed), lmw and lm.  A NEW prefix
    p + (c,), c != sep   is proposed only if part + (c,) is a prefix of a pronunciation; lmw, lm and words carry over
    p + (sep,)           is proposed only if part is a pronunciation; w* = argmax over its words of ln P_lm(w | words), exact ties to the
                         first (lowest id);  lmw' = lmw + (lm_weight * ln P(w*) + word_bonus),  lm' = lm + ln P(w*),  words' = words + (w*,)
and the W entries with the largest key = total + lmw survive (an entry whose total is -inf never does; exact ties keep ctc_beam_ref's
order; a rejected candidate has no entry).  Without a model every ln P is 0.  After the last frame a hypothesis with part == () is
complete, one whose part is a pronunciation is closed as if by a sep without acoustic term and is complete, any other is incomplete
(no closing term, the unfinished word is not emitted); with use_eos complete hypotheses add lm_weight * ln P_lm(</s> | words).  The final
order: complete before incomplete, then the final key descending, then the order of the last selection.

`dtype` is the arithmetic of lp, of every logaddexp and of the lmw / lm sums and keys (the float64 score is rounded to `dtype` first).
Besides frame_gap / final_gap / ties (ctc_lm_ref's, on these keys; final gaps and ties between neighbours of equal completeness) the run
reports word_gap: the smallest non-zero difference between the best and the second-best homophone at every word end an entry that was
kept (or a final closing) took, with ("word", t, prefix) in ties where that difference is exactly 0."""
import numpy as np

from tests.ctc_beam_ref import _lae, candidates


def lexicon_dicts(lexicon):
    """a utils.lexicon.Lexicon -> (prons {pronunciation: [word ids]}, prefixes set): what this file decodes with"""
    return {p: list(ws) for p, ws in lexicon.pronunciations.items()}, lexicon.prefixes()


def choose(prons, lm, part, words, dt):
    """the word a sep behind (part, words) closes -> (w*, ln P(w*) in dt, gap to the second best as float, inf with one word)"""
    start = tuple(lm.start_context) if lm is not None else ()
    sc = [dt(lm.score(start + words, w)) if lm is not None else dt(0.0) for w in prons[part]]
    best = max(range(len(sc)), key=lambda i: (float(sc[i]), -i))
    rest = [float(sc[best]) - float(s) for i, s in enumerate(sc) if i != best]
    return prons[part][best], sc[best], min(rest, default=np.inf)


def search_one(x, prons, prefixes, lm, blank, sep, W, K, lm_weight=1.0, word_bonus=0.0, use_eos=True, dtype=np.float64, stats=None):
    """x [T_b, C] raw logits of one sample -> (hyps, frame_gap, word_gap, ties): hyps = the final beam [(prefix, am, lm, total, words,
    complete)] in the final order.  stats (a dict): "beams" (the prefixes after every frame), "rejected" (candidates without a key, per
    frame), "table" (entries with a key, per frame), "choices" [(part, words, w*)] of every kept word end, "closed" / "incomplete" (prefixes of the final beam)."""
    dt = np.dtype(dtype).type
    NEG = dt(-np.inf)
    w, bonus = dt(lm_weight), dt(word_bonus)
    beam = [((), dt(0.0), NEG, dt(0.0), dt(0.0), (), ())]          # (prefix, pb, pnb, lmw, lm, part, words) in the order of the last selection
    frame_gap, word_gap, ties = np.inf, np.inf, []
    for t in range(x.shape[0]):
        raw = x[t]
        row = raw.astype(dtype)
        m = row.max()
        lp = row - (m + np.log(np.exp(row - m).sum(dtype=dtype)))
        cand = candidates(raw, blank, K)
        rank = {c: k for k, c in enumerate(cand)}
        where = {r[0]: j for j, r in enumerate(beam)}
        kids = {}
        for q in where:
            if q:
                kids.setdefault(q[:-1], []).append(q[-1])
        new = {}                                                   # prefix -> [pb, pnb, place, lmw, lm, part, words, homophone gap or None]
        rejected = 0

        def add(p, pb, pnb, place, rest):
            o = new.get(p)
            if o is None:
                new[p] = [pb, pnb, place] + list(rest)
            else:
                o[0], o[1] = _lae(o[0], pb), _lae(o[1], pnb)

        for j, (p, pb, pnb, lmw, lms, part, words) in enumerate(beam):
            tot = _lae(pb, pnb)
            add(p, tot + lp[blank], NEG, j, (lmw, lms, part, words, None))
            e = p[-1] if p else None
            if p:
                add(p, NEG, pnb + lp[e], j, (lmw, lms, part, words, None))
            for c in cand + [c for c in kids.get(p, ()) if c not in rank]:
                q = p + (c,)
                flow = (pb if c == e else tot) + lp[c]
                if q in where:                                     # a resident prefix carries its own values
                    add(q, NEG, flow, where[q], beam[where[q]][3:] + (None,))
                    continue
                place = W + j * len(cand) + rank[c]
                if c != sep:
                    if part + (c,) in prefixes:
                        add(q, NEG, flow, place, (lmw, lms, part + (c,), words, None))
                    else:
                        rejected += 1
                elif part in prons:
                    wd, s, gap = choose(prons, lm, part, words, dt)
                    add(q, NEG, flow, place, (lmw + (w * s + bonus), lms + s, (), words + (wd,), (gap, part, words, wd)))
                else:
                    rejected += 1
        table = [(p, v[0], v[1], _lae(v[0], v[1])) + tuple(v[2:]) for p, v in new.items()]
        table = [r + (r[3] + r[5],) for r in table if r[3] > NEG]  # (p, pb, pnb, total, place, lmw, lm, part, words, word end, key)
        table = [r for r in table if r[10] > NEG]
        table.sort(key=lambda r: (-float(r[10]), r[4]))
        if len(table) > W:
            gap = float(table[W - 1][10]) - float(table[W][10])
            if gap == 0.0:
                ties.append(("frame", t))
            else:
                frame_gap = min(frame_gap, gap)
        for r in table[:W]:
            if r[9] is not None:
                gap, part, words, wd = r[9]
                if gap == 0.0:
                    ties.append(("word", t, r[0]))
                else:
                    word_gap = min(word_gap, gap)
                if stats is not None:
                    stats.setdefault("choices", []).append((part, words, wd))
        beam = [(r[0], r[1], r[2], r[5], r[6], r[7], r[8]) for r in table[:W]]
        if stats is not None:
            stats.setdefault("table", []).append(len(table))
            stats.setdefault("beams", []).append([r[0] for r in beam])
            stats.setdefault("rejected", []).append(rejected)
    start = tuple(lm.start_context) if lm is not None else ()
    final = []
    for p, pb, pnb, lmw, lms, part, words in beam:
        am = _lae(pb, pnb)
        done = part == ()
        if not done and part in prons:
            wd, s, gap = choose(prons, lm, part, words, dt)
            if gap == 0.0:
                ties.append(("word", x.shape[0], p))
            else:
                word_gap = min(word_gap, gap)
            lmw, lms, words, done = lmw + (w * s + bonus), lms + s, words + (wd,), True
            if stats is not None:
                stats.setdefault("closed", []).append(p)
                stats.setdefault("choices", []).append((part, words[:-1], wd))
        elif not done and stats is not None:
            stats.setdefault("incomplete", []).append(p)
        key = am + lmw
        if use_eos and done:
            s = dt(lm.score(start + words, lm.eos)) if lm is not None else dt(0.0)
            key, lms = key + w * s, lms + s
        final.append((p, float(am), float(lms), float(key), words, done))
    final.sort(key=lambda r: (not r[5], -r[3]))                    # stable
    ties += [("final", i) for i in range(len(final) - 1) if final[i][5] == final[i + 1][5] and final[i][3] == final[i + 1][3]]
    return final, frame_gap, word_gap, ties


def beam_search(logits, prons, prefixes, lm=None, sep=1, input_lengths=None, blank=0, beam_width=8, topk=None, nbest=1, lm_weight=1.0,
                word_bonus=0.0, use_eos=True, pad=-100, dtype=np.float64, stats=None):
    """logits [B, T, C] -> dict: words int64 [B, nbest, (T + 1) // 2] and ids int64 [B, nbest, T] padded with `pad`, word_lengths, lengths
    int64 [B, nbest], am / lm / total float64 [B, nbest] (-inf and lengths 0 for a slot without hypothesis), complete uint8 [B, nbest],
    hyps (per sample the whole final beam), frame_gap, final_gap, word_gap [B] and ties (per sample, see search_one)."""
    x = np.asarray(logits)
    B, T, C = x.shape
    K = min(32, C - 1) if topk is None else min(int(topk), C - 1)
    words = np.full((B, nbest, (T + 1) // 2), pad, dtype=np.int64)
    ids = np.full((B, nbest, T), pad, dtype=np.int64)
    word_lengths, lengths = np.zeros((B, nbest), dtype=np.int64), np.zeros((B, nbest), dtype=np.int64)
    complete = np.zeros((B, nbest), dtype=np.uint8)
    am, lms, total = (np.full((B, nbest), -np.inf) for _ in range(3))
    hyps_all, ties_all = [], []
    frame_gap, final_gap, word_gap = np.full(B, np.inf), np.full(B, np.inf), np.full(B, np.inf)
    for b in range(B):
        tb = T if input_lengths is None else min(max(int(input_lengths[b]), 0), T)
        st = None if stats is None else stats.setdefault(b, {})
        hyps, frame_gap[b], word_gap[b], ties = search_one(x[b, :tb], prons, prefixes, lm, blank, sep, beam_width, K, lm_weight, word_bonus,
                                                           use_eos, dtype, st)
        hyps_all.append(hyps)
        ties_all.append(ties)
        final_gap[b] = min([hyps[i][3] - hyps[i + 1][3] for i in range(len(hyps) - 1)
                            if hyps[i][5] == hyps[i + 1][5] and hyps[i][3] != hyps[i + 1][3]], default=np.inf)
        for h, (p, a, l, k, ws, done) in enumerate(hyps[:nbest]):
            ids[b, h, :len(p)] = p
            lengths[b, h] = len(p)
            words[b, h, :len(ws)] = ws
            word_lengths[b, h] = len(ws)
            am[b, h], lms[b, h], total[b, h], complete[b, h] = a, l, k, done
    return dict(words=words, word_lengths=word_lengths, ids=ids, lengths=lengths, am=am, lm=lms, total=total, complete=complete, hyps=hyps_all,
                ties=ties_all, frame_gap=frame_gap, final_gap=final_gap, word_gap=word_gap)


def brute_force(x, prons, prefixes, lm, blank, sep, lm_weight=1.0, word_bonus=0.0, use_eos=True):
    """x [T, C] -> {labelling: (am, lm, total, words, complete)} over all C^T alignments in float64, for every labelling the lexicon admits
    (each label extends a pronunciation prefix, each sep stands behind a pronunciation)"""
    from tests.ctc_beam_ref import brute_force as am_brute_force
    start = tuple(lm.start_context) if lm is not None else ()
    out = {}
    for p, am in am_brute_force(x, blank).items():
        part, words, s, ok = (), (), 0.0, True
        for c in p:
            if c != sep and part + (c,) in prefixes:
                part = part + (c,)
            elif c == sep and part in prons:
                wd, lp, _ = choose(prons, lm, part, words, np.float64)
                part, words, s = (), words + (wd,), s + lp
            else:
                ok = False
                break
        if not ok:
            continue
        done = part == ()
        if not done and part in prons:
            wd, lp, _ = choose(prons, lm, part, words, np.float64)
            words, s, done = words + (wd,), s + lp, True
        if use_eos and done and lm is not None:
            s += lm.score(start + words, lm.eos)
        out[p] = (am, s, am + lm_weight * s + word_bonus * len(words), words, done)
    return out
