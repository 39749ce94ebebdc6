"""The cases tests/test_ctc_lm_cpu.py and tests/test_ctc_lm_gpu.py share: the smallest shapes at which each mechanism of the CTC prefix
beam search with n-gram shallow fusion (fk_ctc_beam_search_lm, csrc/ctc.hip) can fail, each with its float64 result from
tests/ctc_lm_ref.py.  The rule is that of tests/ctc_beam_cases.py, on the FUSED keys.

Logits are 2 * randn with + 3 on the blank column, stored as a view into NaN-padded rows; sample 0 has T_b = T, the others T_b in
[T / 2, T].  The language models are interpolated Witten-Bell models (NGramLM.from_corpus) of seeded Zipf-distributed sequences
(utils.ngram.zipf_sequences); the float64 yardstick scores them with NGramLM.score, the dictionary definition.

make() asserts a MARGIN for every sample: with e32 the largest difference of am, lm or total between the float32 and the float64 run of
the restatement on that sample, the smallest gap between the W-th and the (W + 1)-th key over all frames, and between neighbouring final
keys, is at least 16 * e32, with exact ties in the same places in both runs.  The kernel is allowed 4 * e32 per score, two entries that
swap places need 8 * e32: a factor of two is left.  The seeds below were chosen on the CPU so that every sample of every case passes;
no sample is left out anywhere.  What else make() asserts is in the table."""
import functools

import numpy as np
import torch

from frankenstein_amd.utils.ngram import NGramLM, zipf_sequences
from tests import ctc_beam_ref as BR
from tests import ctc_lm_ref as LR

PAD = -100
MARGIN = 16.0

#        B,   T,     C, blank, row stride,  W,  K, nbest, order, lm_weight, length_bonus, seed
CASES = {
    "x": (2,   4,     3,     2,     3, 32,  2, 32, 3, 0.8,  0.5, 0),   # nothing pruned: order and totals equal brute force + LM
    "s": (4,  12,     5,     0,     5,  4,  4,  2, 2, 0.8,  0.5, 0),   # short samples, one with T_b = 0; W below the table
    "b": (2,  16,     6,     0,     6,  4,  3,  4, 4, 0.8,  0.5, 1),   # order 4 from a handful of sequences: most look-ups back off >= 2 levels
    "m": (3,  40,   300,   299,   304,  8,  8,  8, 3, 0.8,  0.5, 2),   # most classes unseen (the unigram floor); last labels outside the candidates
    "v": (4,  32, 50258, 50257, 50258,  5, 20,  5, 3, 0.5,  1.0, 0),   # the project's vocabulary; a table with probe lengths > 1
    "t": (2,  48,    41,     0,    41, 32, 32, 32, 3, 0.8,  0.5, 1),   # the top of the envelope: 1024 look-ups per frame
    "l": (2, 200,    41,     0,    48,  8, 12,  1, 3, 0.8,  0.5, 29),  # a long recursion
    "r": (2,  24,     4,     0,     4,  3,  2,  3, 2, 0.8,  0.5, 20),  # a prefix returns under a descendant that stayed: lmw and state come back
    "p": (1,  10,     6,     0,     6,  2,  2,  2, 3, 1.5,  0.0, 0),   # the fused best labelling is not in the plain search's final beam
    "e": (4,  12,     5,     0,     5,  4,  4,  4, 2, 1.5,  0.0, 0),   # as "s": the end of sentence changes the final order ("e_noeos": without)
}

#        sequences, (shortest, longest), distinct classes (None: all), seed
CORPORA = {
    "x": (30, (1, 4), None, 7), "s": (40, (2, 8), None, 7), "b": (5, (3, 6), None, 7), "m": (200, (3, 12), 20, 7),
    "v": (2000, (5, 20), 5000, 7), "t": (300, (5, 30), None, 7), "l": (300, (5, 30), None, 7), "r": (20, (2, 8), None, 7),
    "p": (40, (2, 8), 3, 7), "e": (40, (2, 8), None, 7),
}


@functools.lru_cache(maxsize=None)
def model(name):
    """the case's language model"""
    B, T, C, blank, ld, W, K, nbest, order, lw, bonus, seed = CASES[name]
    n, length, types, lm_seed = CORPORA[name]
    return NGramLM.from_corpus(zipf_sequences(n, C, blank, length, lm_seed, n_types=types), order, C)


def generate(name, seed):
    """-> (store fp32 [B, T, row stride] with NaN behind column C, input_lengths int64 [B])"""
    B, T, C, blank, ld = CASES[name][:5]
    store = torch.full((B, T, ld), float("nan"))
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    Tb = [T] + [int(rng.integers(T // 2, T + 1)) for _ in range(B - 1)]
    if name in ("s", "e"):
        Tb[2] = 0
    g = torch.Generator().manual_seed(8642 + 1000 * seed + sum(map(ord, name)))
    x = 2.0 * torch.randn((B, T, C), generator=g)
    x[:, :, blank] += 3.0
    store[:, :, :C] = x
    return store, torch.tensor(Tb, dtype=torch.int64)


def measure(x, il, lm, blank, W, K, nbest, lw, bonus, use_eos, stats=None):
    """the float64 and the float32 run of the restatement -> (ref64, e32 [B], margin [B]); e32 is inf for a sample whose float32 run ends
    with other prefixes or another order, or has its exact ties elsewhere"""
    ref = LR.beam_search(x, lm, il, blank, W, K, nbest, lw, bonus, use_eos, PAD, np.float64, stats)
    r32 = LR.beam_search(x, lm, il, blank, W, K, nbest, lw, bonus, use_eos, PAD, np.float32)
    B = x.shape[0]
    e32, margin = np.zeros(B), np.zeros(B)
    for b in range(B):
        h64, h32 = ref["hyps"][b], r32["hyps"][b]
        if [r[0] for r in h64] != [r[0] for r in h32] or ref["ties"][b] != r32["ties"][b]:
            e32[b] = np.inf
            continue
        e32[b] = max(abs(u - v) for r, q in zip(h64, h32) for u, v in zip(r[1:], q[1:]))
        margin[b] = min(ref["frame_gap"][b], ref["final_gap"][b])
    return ref, e32, margin


def returns_under_a_descendant(beams):
    """beams: the beam after every frame -> how often a prefix enters the beam that was in it before, left, and is the start of a prefix
    that stayed (the kernel must give it its node, its lmw and its LM state back)"""
    seen, prev, n = {()}, {()}, 0
    for cur in map(set, beams):
        n += sum(1 for p in cur - prev if p in seen and any(q != p and q[:len(p)] == p for q in cur))
        seen |= cur
        prev = cur
    return n


@functools.lru_cache(maxsize=None)
def make(key):
    """key: a case name, "v_bf16" (the logits of "v" rounded to bf16) or "e_noeos" (case "e" without the end of sentence) ->
    dict(logits fp32 [B, T, C] (a view into [B, T, row stride] storage), input_lengths, blank, ld, W, K, nbest, lm (the NGramLM),
    lm_weight, length_bonus, use_eos, ref (the float64 result of tests/ctc_lm_ref.beam_search), e32 [B]).  Cached: read-only."""
    name = key.split("_")[0]
    B, T, C, blank, ld, W, K, nbest, order, lw, bonus, seed = CASES[name]
    use_eos = not key.endswith("_noeos")
    store, il = generate(name, seed)
    if key.endswith("_bf16"):
        store = store.to(torch.bfloat16).float()
    logits = store[:, :, :C]
    x = logits.numpy()
    lm = model(name)
    stats = {}
    ref, e32, margin = measure(x, il.numpy(), lm, blank, W, K, nbest, lw, bonus, use_eos, stats)
    assert np.all(np.isfinite(e32)) and np.all(margin >= MARGIN * e32), (key, e32, margin)
    if name == "b":
        levels = np.array([n for b in stats for n in stats[b].get("levels", [])])
        assert (levels >= 2).mean() > 0.5, (key, np.bincount(levels))
    if name == "m":
        levels = np.array([n for b in stats for n in stats[b].get("levels", [])])
        assert (levels == order - 1).mean() > 0.5, (key, np.bincount(levels))
        tb = int(il[0])                                              # a resident prefix whose last label is no candidate of the last frame
        assert any(p and p[-1] not in BR.candidates(x[0, tb - 1], blank, K) for p in stats[0]["beams"][tb - 2]), key
    if name == "v":
        assert lm.compile().max_probe > 1, key
    if name == "r":
        assert returns_under_a_descendant(stats[0]["beams"]) > 0, key
    if name == "p":                                                  # no rescoring of the plain beam could have found the fused best
        plain = BR.beam_search(x, il.numpy(), blank, W, K, W, PAD, np.float64)
        assert all(ref["hyps"][b][0][0] not in [p for p, _ in plain["hyps"][b]] for b in range(B)), key
    if key == "e":
        off = make("e_noeos")["ref"]
        assert any([r[0] for r in ref["hyps"][b]] != [r[0] for r in off["hyps"][b]] and
                   sorted(r[0] for r in ref["hyps"][b]) == sorted(r[0] for r in off["hyps"][b]) for b in range(B)), key
    return dict(name=key, logits=logits, input_lengths=il, blank=blank, ld=ld, W=W, K=K, nbest=nbest, lm=lm, lm_weight=lw, length_bonus=bonus,
                use_eos=use_eos, ref=ref, e32=e32)
