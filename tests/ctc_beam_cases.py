"""The cases tests/test_ctc_beam_cpu.py and tests/test_ctc_beam_gpu.py share: the smallest shapes at which each mechanism of the CTC
prefix beam search (fk_ctc_beam_search, csrc/ctc.hip) can fail, each with its float64 result from tests/ctc_beam_ref.py.

Logits are 2 * randn with + 3 on the blank column (so that the best path and the best labelling disagree), stored as a view into
NaN-padded rows.  Sample 0 has T_b = T, the others T_b in [T / 2, T] (hand-picked where a case needs a particular sample).

make() asserts a MARGIN for every sample, so that a comparison of ids on the GPU cannot hinge on rounding: with e32 the largest score
difference between the float32 and the float64 run of the restatement on that sample, the smallest gap between the W-th and the
(W + 1)-th total over all frames, and between neighbouring totals of the final beam, is at least 16 * e32.  The kernel is allowed
4 * e32 per score, two entries that swap places need 8 * e32: a factor of two is left.  The seeds below were chosen on the CPU so that
every sample of every case passes; no sample is left out anywhere.  make() also asserts that "s", "m", "t" and "l" contain a sample
whose best hypothesis is not the greedy one, and that in "r" a prefix returns to the beam under a descendant that stayed.

An exact tie is no gap: two candidates with equal logits behind one parent are the same sum of the same addends in every arithmetic,
and the fixed order of the semantics decides them (the lower parent slot, then the better candidate).  The restatement lists where they
occur; make() asserts that the float32 and the float64 run have them in the same places and takes the margin over the other gaps.  The
example "g" has one ("ab" and "ba", competing for the fourth place), the bf16-rounded logits of "v_bf16" have them in most frames."""
import functools

import numpy as np
import torch

from tests import ctc_beam_ref as BR
from tests import ctc_ref as R

PAD = -100

#        B,   T,     C, blank, row stride,  W,  K, nbest, seed
CASES = {
    "x": (2,   4,     3,     2,     3, 32,  2, 32, 0),    # exhaustive: at most 31 prefixes, nothing pruned
    "g": (1,   2,     3,     0,     3,  4,  2,  4, None),  # the example: greedy decodes "", the best labelling is "a"
    "s": (4,  12,     5,     0,     5,  4,  4,  2, 0),    # short samples, one with T_b = 0; W smaller than the table
    "m": (3,  80,   300,   299,   304,  8,  8,  8, 9),    # C no multiple of the vector width, padded rows, last labels outside the candidates
    "v": (4,  32, 50258, 50257, 50258,  5, 20,  5, 1),    # the project's vocabulary and its beam defaults
    "t": (2,  48,    41,     0,    41, 32, 32, 32, 4),    # the top of the envelope: 1056 entries per selection
    "l": (2, 200,    41,     0,    48,  8, 12,  1, 31),    # a long recursion: node table and backtrack over hundreds of frames
    "r": (2,  24,     4,     0,     4,  3,  2,  3, 21),    # a prefix leaves the beam and comes back while a longer one built on it stayed
}
DIFFERS_FROM_GREEDY = ("s", "m", "t", "l")
MARGIN = 16.0


def generate(name, seed):
    """-> (store fp32 [B, T, row stride] with NaN behind column C, input_lengths int64 [B])"""
    B, T, C, blank, ld, W, K, nbest, _ = CASES[name]
    store = torch.full((B, T, ld), float("nan"))
    if name == "g":
        store[:, :, :C] = torch.log(torch.tensor([0.40, 0.35, 0.25]))
        return store, torch.tensor([T], dtype=torch.int64)
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    Tb = [T] + [int(rng.integers(T // 2, T + 1)) for _ in range(B - 1)]
    if name == "s":
        Tb[2] = 0
    g = torch.Generator().manual_seed(4321 + 1000 * seed + sum(map(ord, name)))
    x = 2.0 * torch.randn((B, T, C), generator=g)
    x[:, :, blank] += 3.0
    store[:, :, :C] = x
    return store, torch.tensor(Tb, dtype=torch.int64)


def measure(x, il, blank, W, K, nbest):
    """the float64 and the float32 run of the restatement on logits x -> (ref64, e32 [B], margin [B]); margin = the smaller of the two
    gaps; e32 is inf for a sample whose float32 run ends with other prefixes or has its exact ties elsewhere"""
    ref = BR.beam_search(x, il, blank, W, K, nbest, PAD, np.float64)
    r32 = BR.beam_search(x, il, blank, W, K, nbest, PAD, np.float32)
    B = x.shape[0]
    e32, margin = np.zeros(B), np.zeros(B)
    for b in range(B):
        h64, h32 = ref["hyps"][b], r32["hyps"][b]
        if [p for p, _ in h64] != [p for p, _ in h32] or ref["ties"][b] != r32["ties"][b]:
            e32[b] = np.inf
            continue
        e32[b] = max(abs(s - q) for (_, s), (_, q) in zip(h64, h32))
        margin[b] = min(ref["frame_gap"][b], ref["final_gap"][b])
    return ref, e32, margin


def returns_under_a_descendant(x, blank, W, K):
    """x [T_b, C] -> how often a prefix enters the beam that was in it before, left, and is the start of a prefix that stayed: the kernel
    must give it the identity its descendant still points to, or the descendant is no longer recognised as its child"""
    seen, prev, n = {()}, {()}, 0
    for t in range(1, x.shape[0] + 1):
        cur = {p for p, _ in BR.search_one(x[:t], blank, W, K)[0]}
        n += sum(1 for p in cur - prev if p in seen and any(q != p and q[:len(p)] == p for q in cur))
        seen |= cur
        prev = cur
    return n


def greedy(x, il, blank):
    return R.collapse(np.asarray(x).argmax(-1), il, blank=blank, pad=PAD)


@functools.lru_cache(maxsize=None)
def make(key):
    """key: a case name, or "v_bf16" (the logits of "v" rounded to bf16) -> dict(logits fp32 [B, T, C] (a view into [B, T, row stride]
    storage), input_lengths, blank, ld, W, K, nbest, ref (the float64 result of tests/ctc_beam_ref.beam_search), e32 [B]).  Cached: treat
    everything as read-only."""
    name = key[:-5] if key.endswith("_bf16") else key
    B, T, C, blank, ld, W, K, nbest, seed = CASES[name]
    store, il = generate(name, seed)
    if key.endswith("_bf16"):
        store = store.to(torch.bfloat16).float()
    logits = store[:, :, :C]
    x = logits.numpy()
    ref, e32, margin = measure(x, il.numpy(), blank, W, K, nbest)
    assert np.all(np.isfinite(e32)) and np.all(margin >= MARGIN * e32), (key, e32, margin)
    if name in DIFFERS_FROM_GREEDY:
        ids, lens = greedy(x, il.numpy(), blank)
        assert any(int(lens[b]) != int(ref["lengths"][b, 0]) or not np.array_equal(ids[b], ref["ids"][b, 0]) for b in range(B)), key
    if name == "r":
        assert returns_under_a_descendant(x[0, :int(il[0])], blank, W, K) > 0, key
    return dict(name=key, logits=logits, input_lengths=il, blank=blank, ld=ld, W=W, K=K, nbest=nbest, ref=ref, e32=e32)
