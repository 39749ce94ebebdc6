"""The cases tests/test_ctc_lex_cpu.py and tests/test_ctc_lex_gpu.py share: the smallest shapes at which each mechanism of the
lexicon-constrained CTC prefix beam search (fk_ctc_beam_search_lex, csrc/ctc.hip) can fail, each with its float64 result from
tests/ctc_lex_ref.py.  The rule is that of tests/ctc_lm_cases.py and its MARGIN, on these keys and on the homophone choices.

Logits are 2 * randn with + 3 on the blank column and + SEP_BOOST on the separator (so that words end), stored as a view into NaN-padded
rows; sample 0 has T_b = T, the others T_b in [T / 2, T], case "s" has one T_b = 0.  The lexicons are explicit or seeded
(utils.lexicon.zipf_lexicon), the word models interpolated Witten-Bell models (NGramLM.from_corpus) of explicit or seeded Zipf-distributed
word sequences; the float64 yardstick scores them with NGramLM.score.

make() asserts a MARGIN for every sample: with e32 the largest difference of am, lm or total between the float32 and the float64 run of
the restatement on that sample, the smallest gap between the W-th and the (W + 1)-th key over all frames, between neighbouring final
keys, and between the best and the second-best homophone at every word end a kept entry took, is at least 16 * e32, with exact ties in
the same places in both runs.  The seeds below were chosen on the CPU so that every sample of every case passes; no sample is left out
anywhere.  What else make() asserts is in the table."""
import functools

import numpy as np
import torch

from frankenstein_amd.utils.lexicon import Lexicon, zipf_lexicon
from frankenstein_amd.utils.ngram import NGramLM, zipf_sequences
from tests import ctc_beam_ref as BR
from tests import ctc_lex_ref as XR
from tests.ctc_lm_cases import MARGIN, PAD, returns_under_a_descendant

SEP_BOOST = 1.5

#        B,   T,  C, blank, sep, row stride,  W,  K, nbest, lexicon, word model, lm_weight, word_bonus, seed
CASES = {
    "x": (2,   5,  4,     3,   0,   4, 32,  3, 32, "x",   "x",  0.8,  0.5, 0),   # nothing pruned: order and totals equal brute force
    "s": (4,  12,  6,     0,   1,   6,  4,  4,  2, "s",   None, 1.0,  0.5, 0),   # short samples, one with T_b = 0; no word model
    "h": (2,  16,  5,     0,   1,   5,  6,  4,  6, "h",   "h",  1.0,  0.0, 0),   # three homophones, resolved by the context, not always the lowest id
    "c": (2,  14,  6,     0,   1,   6,  6,  4,  6, "c",   "c",  0.8,  0.5, 0),   # closed without sep; an incomplete one behind a complete one of smaller key
    "j": (1,  10,  6,     0,   1,   6,  2,  3,  2, "c",   "c",  0.8,  0.5, 0),   # the lexicon rejects what the plain search keeps; its best is not in the plain beam
    "r": (2,  24,  5,     0,   1,   5,  3,  2,  3, "h",   "h",  0.8,  0.5, 1),   # a prefix returns under a descendant that stayed: node, lmw, state, count come back
    "p": (2,  24, 41,     0,   1,  41,  8, 12,  8, "big", "big", 0.8, 0.5, 0),   # ~2000 words, order-3 word model: a trie table with probe lengths > 1
    "t": (2,  48, 41,     0,   1,  41, 32, 32, 32, "big", "big", 0.8, 0.5, 1),   # the top of the envelope
    "l": (2, 200, 41,     0,   1,  48,  8, 12,  1, "big", "big", 0.8, 0.5, 0),   # a long recursion
}


@functools.lru_cache(maxsize=None)
def lexicon(name):
    if name == "x":                                                # classes 1, 2; two homophones on (1,); (2,) ends no word
        return Lexicon([("a", (1,)), ("ah", (1,)), ("ab", (1, 2)), ("ba", (2, 1))])
    if name == "h":                                                # classes 2, 3, 4; three homophones on (2,)
        return Lexicon([("to", (2,)), ("too", (2,)), ("two", (2,)), ("go", (3,)), ("at", (4,)), ("tog", (2, 3))])
    if name == "s":
        return zipf_lexicon(12, 6, 0, 1, (1, 3), 3, 0.2)
    if name == "c":
        return zipf_lexicon(10, 6, 0, 1, (2, 3), 5, 0.2)
    return zipf_lexicon(2000, 41, 0, 1, (1, 4), 11, 0.1)


@functools.lru_cache(maxsize=None)
def model(name):
    """the case's word model (None: none)"""
    if name is None:
        return None
    V = len(lexicon(name))
    if name == "x":
        return NGramLM.from_corpus([(0, 3), (1, 2), (3, 1), (2,), (1, 3, 0)], 2, V)
    if name == "h":                                                # "to" at the start, "too" behind "go", "two" behind "at"
        return NGramLM.from_corpus([(0, 3, 1, 4, 2), (3, 1), (4, 2), (0, 4, 2, 3, 1), (0, 5), (3, 1, 4, 2), (0, 3, 1)] * 2, 2, V)
    if name == "c":
        return NGramLM.from_corpus(zipf_sequences(40, V + 1, V, (2, 6), 7), 2, V)
    return NGramLM.from_corpus(zipf_sequences(400, V + 1, V, (3, 10), 7), 3, V)


def generate(name, seed):
    """-> (store fp32 [B, T, row stride] with NaN behind column C, input_lengths int64 [B])"""
    B, T, C, blank, sep, ld = CASES[name][:6]
    store = torch.full((B, T, ld), float("nan"))
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    Tb = [T] + [int(rng.integers(T // 2, T + 1)) for _ in range(B - 1)]
    if name == "s":
        Tb[2] = 0
    if name == "x":
        Tb[1] = T - 1
    g = torch.Generator().manual_seed(97531 + 1000 * seed + sum(map(ord, name)))
    x = 2.0 * torch.randn((B, T, C), generator=g)
    x[:, :, blank] += 3.0
    x[:, :, sep] += SEP_BOOST
    store[:, :, :C] = x
    return store, torch.tensor(Tb, dtype=torch.int64)


def measure(x, il, prons, prefixes, lm, blank, sep, W, K, nbest, lw, bonus, use_eos=True, stats=None):
    """the float64 and the float32 run of the restatement -> (ref64, e32 [B], margin [B]); e32 is inf for a sample whose float32 run ends
    with other hypotheses, other words or another order, or has its exact ties elsewhere"""
    ref = XR.beam_search(x, prons, prefixes, lm, sep, il, blank, W, K, nbest, lw, bonus, use_eos, PAD, np.float64, stats)
    r32 = XR.beam_search(x, prons, prefixes, lm, sep, il, blank, W, K, nbest, lw, bonus, use_eos, PAD, np.float32)
    B = x.shape[0]
    e32, margin = np.zeros(B), np.zeros(B)
    for b in range(B):
        h64, h32 = ref["hyps"][b], r32["hyps"][b]
        if [(r[0], r[4], r[5]) for r in h64] != [(r[0], r[4], r[5]) for r in h32] or ref["ties"][b] != r32["ties"][b]:
            e32[b] = np.inf
            continue
        e32[b] = max(abs(u - v) for r, q in zip(h64, h32) for u, v in zip(r[1:4], q[1:4]))
        margin[b] = min(ref["frame_gap"][b], ref["final_gap"][b], ref["word_gap"][b])
    return ref, e32, margin


def admitted(p, prons, prefixes, sep):
    """whether the lexicon admits the labelling p"""
    part = ()
    for c in p:
        if c != sep and part + (c,) in prefixes:
            part = part + (c,)
        elif c == sep and part in prons:
            part = ()
        else:
            return False
    return True


def mechanism(name, case, ref, stats):
    """what the table says the case is for; AssertionError when it does not occur"""
    B, T, C, blank, sep, ld, W, K, nbest, lex_name, lm_name, lw, bonus, seed = CASES[name]
    x, il = case["logits"].numpy(), case["input_lengths"].numpy()
    prons, prefixes = case["prons"], case["prefixes"]
    if name == "x":
        assert all(n <= W for b in stats for n in stats[b].get("table", [])) and K == C - 1, name
    if name == "s":
        assert case["lm"] is None and int(il[2]) == 0 and ref["hyps"][2] == [((), 0.0, 0.0, 0.0, (), True)], name
    if name == "h":
        picks = {}
        for b in stats:
            for part, words, wd in stats[b].get("choices", []):
                if len(prons[part]) >= 3:
                    picks.setdefault(part, set()).add(wd)
        assert any(len(v) >= 2 and max(v) != min(prons[part]) for part, v in picks.items()), (name, picks)
    if name == "c":
        assert any(stats[b].get("closed") for b in stats), name
        assert any(not ref["hyps"][b][i][5] and any(q[5] and q[3] < ref["hyps"][b][i][3] for q in ref["hyps"][b][:i])
                   for b in range(B) for i in range(len(ref["hyps"][b]))), name
    if name == "j":
        plain = BR.beam_search(x, il, blank, W, K, W, PAD, np.float64)
        assert all(any(not admitted(p, prons, prefixes, sep) for p, _ in plain["hyps"][b]) for b in range(B)), name
        assert all(ref["hyps"][b][0][0] not in [p for p, _ in plain["hyps"][b]] for b in range(B)), name
        assert sum(stats[0]["rejected"]) > 0, name
    if name == "r":
        assert returns_under_a_descendant(stats[0]["beams"]) > 0, name
    if name == "p":
        assert lexicon(lex_name).compile().max_probe > 1 and model(lm_name).order == 3 and len(lexicon(lex_name)) >= 1900, name
    if name == "t":
        assert W == 32 and K == 32 and any(len(bm) == W for b in stats for bm in stats[b]["beams"]), name
    if name == "l":
        assert T >= 200 and int(il[0]) == T, name


def build(key, seed=None):
    """make() for a given seed (None: the table's); raises AssertionError where the margin rule or the mechanism fails"""
    name = key.split("_")[0]
    B, T, C, blank, sep, ld, W, K, nbest, lex_name, lm_name, lw, bonus, table_seed = CASES[name]
    store, il = generate(name, table_seed if seed is None else seed)
    if key.endswith("_bf16"):
        store = store.to(torch.bfloat16).float()
    logits = store[:, :, :C]
    lex, lm = lexicon(lex_name), model(lm_name)
    prons, prefixes = XR.lexicon_dicts(lex)
    stats = {}
    ref, e32, margin = measure(logits.numpy(), il.numpy(), prons, prefixes, lm, blank, sep, W, K, nbest, lw, bonus, True, stats)
    assert np.all(np.isfinite(e32)) and np.all(margin >= MARGIN * e32), (key, e32, margin)
    case = dict(name=key, logits=logits, input_lengths=il, blank=blank, sep=sep, ld=ld, W=W, K=K, nbest=nbest, lexicon=lex, prons=prons,
                prefixes=prefixes, lm=lm, lm_weight=lw, word_bonus=bonus, use_eos=True, ref=ref, e32=e32)
    mechanism(name, case, ref, stats)
    return case


@functools.lru_cache(maxsize=None)
def make(key):
    """key: a case name or "p_bf16" (the logits of "p" rounded to bf16) -> dict(logits fp32 [B, T, C] (a view into [B, T, row stride]
    storage), input_lengths, blank, sep, ld, W, K, nbest, lexicon, prons, prefixes, lm (the NGramLM or None), lm_weight, word_bonus, use_eos,
    ref (the float64 result of tests/ctc_lex_ref.beam_search), e32 [B]).  Cached: read-only."""
    return build(key)


KEYS = tuple(CASES) + ("p_bf16",)


@functools.lru_cache(maxsize=None)
def planted():
    """Logits peaked on the pronunciation of a planted word sequence (words of the big lexicon without homophones, two frames a label:
    the label, then the blank) -> dict(logits fp32 [B, T, 41], input_lengths, blank, sep, lexicon, lm, words: the planted lists)"""
    lex, lm = lexicon("big"), model("big")
    lonely = [ws[0] for p, ws in sorted(lex.pronunciations.items()) if len(ws) == 1]
    rng = np.random.default_rng(5)
    words = [[int(w) for w in rng.choice(lonely, size=n, replace=False)] for n in (5, 3)]
    labs = [lex.pronounce(ws, 1) for ws in words]
    T = 2 * max(map(len, labs))
    g = torch.Generator().manual_seed(5)
    x = 0.5 * torch.randn((len(words), T, 41), generator=g)
    for b, lab in enumerate(labs):
        for s, c in enumerate(lab):
            x[b, 2 * s, c] += 12.0
            x[b, 2 * s + 1, 0] += 12.0
    return dict(logits=x, input_lengths=torch.tensor([2 * len(lab) for lab in labs]), blank=0, sep=1, lexicon=lex, lm=lm, words=words)
