"""The cases tests/test_rescore_cpu.py and tests/test_rescore_gpu.py share: the smallest n-best lists at which each mechanism of the LM
rescoring (csrc/rescore.hip, GPT.score_nbest / rescore_nbest) can fail, each with its float64 result from tests/rescore_ref.py.

Model: GPT n_layer = 2, n_embd = 128, n_head = 4, biases on, block_size 64, every weight 0.2 * randn (LayerNorm gains 1 + 0.1 * randn), so
that the LM is far from uniform; V = 307 (no multiple of 64) and, in "big", 50257.  The values are drawn in float32, so the float64
state dict and the model on the GPU hold the same numbers.

A list is a base sentence with single-token substitutions, deletions and insertions (what one beam gives), or random short sentences
where the trie has to be wide.  The acoustic scores are descending (the beam search's order), so the order without the LM is the identity.
ids live in a larger buffer with garbage behind every length and behind every row: strided, and nothing behind a length may be read.

make() asserts for every RANKING case: the smallest non-zero gap between two totals is at least 16 * e32 (e32: the largest difference
between the float32 and the float64 run of the flat restatement); the rescored order is not the identity in at least one sentence (so it
also changes when lm is replaced by 0: the order by the acoustic score alone is the identity); and scoring the packed rows under a plain
causal table (a node seeing a sibling) moves some score by more than 100 x the tolerance of the GPU test.  Seeds were picked on the CPU
so that all of it holds; duplicates with equal acoustic scores are exact ties and are decided by the original index."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ref_models as RM
from tests import rescore_ref as RR

BOS = 50256                   # remapped to V - 1 for the small vocabulary
FLOOR = 8.0 * 2.0 ** -24
MARGIN = 16.0
GARBAGE = -(1 << 40)

#          V,  B,  n,  T, P, eos, max_nodes, seed, (am_weight, lm_weight, length_bonus)
CASES = {
    "one":      (307,   2,  1,  6, 0, False, None, 1, (1.0, 1.0, 0.0)),     # n = 1: nothing to share, nothing to rank
    "edits":    (307,   3,  8, 12, 5, True,  None, 2, (1.0, 0.7, 0.3)),     # duplicates, the empty hypothesis, absent slots, bad tokens, wild lengths
    "plain":    (307,   2,  8,  9, 0, False, None, 3, (1.0, 1.0, 0.0)),     # P = 0, no end-of-text row
    "mid":      (307,   2, 32,  3, 5, True,  None, 4, (1.0, 0.5, 0.0)),     # n = 32, 64 < P + N <= 128
    "wide":     (307,   2, 32,  5, 0, False, None, 5, (1.0, 0.5, 0.0)),     # n = 32, P + N > 128
    "overflow": (307,   2,  6,  6, 3, True,    10, 6, (1.0, 1.0, 0.0)),     # a static capacity: a middle hypothesis does not fit, a later one does
    "big":      (50257, 1,  4,  5, 3, True,  None, 7, (1.0, 1.0, 0.0)),     # the project's vocabulary
}
RANKING = ("edits", "plain", "mid", "wide", "overflow", "big")


def gpt_cfg(V):
    return RM.gpt_config(block_size=64, vocab_size=V, n_layer=2, n_head=4, n_embd=128, dropout=0.0, bias=True)


@functools.lru_cache(maxsize=None)
def state_dict(V):
    """float32 state dict of the test model (keys of GPT.state_dict() without the tied lm_head)"""
    g = torch.Generator().manual_seed(77 + V)
    sd = {}
    for name, shape in RM.gpt_shapes(gpt_cfg(V)).items():
        w = torch.randn(shape, generator=g)
        if name.endswith(("ln_1.weight", "ln_2.weight", "ln_f.weight")):
            sd[name] = 1.0 + 0.1 * w
        else:
            sd[name] = 0.2 * w
    return sd


@functools.lru_cache(maxsize=None)
def state_dict64(V):
    return {k: v.double() for k, v in state_dict(V).items()}


def _edits(rng, base, V, k):
    """k single-edit variants of the token list `base`"""
    out = []
    for _ in range(k):
        s = list(base)
        kind = rng.integers(3)
        pos = int(rng.integers(len(s)))
        if kind == 0:
            s[pos] = int(rng.integers(V - 1))
        elif kind == 1 and len(s) > 1:
            del s[pos]
        else:
            s.insert(pos, int(rng.integers(V - 1)))
        out.append(s)
    return out


def generate(name):
    """-> SimpleNamespace(ids int64 [B, n, T] (a strided view), lengths int64 [B, n], am fp32 [B, n], prefix fp32 [B, P, d] or None)"""
    V, B, n, T, P, _, _, seed, _ = CASES[name]
    rng = np.random.default_rng(500 + seed)
    store = np.full((B, n + 1, T + 3), GARBAGE, dtype=np.int64)
    lengths = np.zeros((B, n), dtype=np.int64)
    am = np.zeros((B, n), dtype=np.float32)
    for b in range(B):
        if name in ("mid", "wide"):                                     # short divergent sentences: a wide trie
            hyps = [[int(t) for t in rng.integers(0, V - 1, size=int(rng.integers(max(1, T - 1), T + 1)))] for _ in range(n)]
            for h in range(1, n, 5):                                    # a few share a first token
                hyps[h][0] = hyps[h - 1][0]
        else:
            base = [int(t) for t in rng.integers(0, V - 1, size=T - 2)]
            hyps = [base] + _edits(rng, base, V, n - 1)
        hyps = [s[:T] for s in hyps]
        if name == "edits":
            if b == 0:
                hyps[3] = list(hyps[1])                                 # a duplicate: an exact tie when the scores are equal too
                hyps[5] = []                                            # the empty hypothesis
                hyps[6] = (hyps[0] + [1, 2, 3])[:T]                     # a length at T
            if b == 1:
                hyps[2] = hyps[2][:2] + [V] + hyps[2][3:]               # a token equal to V
                hyps[4] = hyps[4][:1] + [-1] + hyps[4][2:]              # a negative token inside the length
                hyps[7] = []                                            # an absent slot (score -inf below)
        if name == "overflow":
            hyps = [hyps[0][:4], hyps[0][:3] + [7], [9, 8, 7, 6, 5, 4], hyps[0][:2], hyps[0][:4] + [11], hyps[0][:3] + [7, 5]]
            if b == 1:
                hyps[2], hyps[3] = hyps[3], hyps[2]
        steps = np.abs(rng.standard_normal(n)).astype(np.float32) * 1.5 + 0.05
        am[b] = -np.cumsum(steps) - 2.0
        for h, s in enumerate(hyps):
            store[b, h, :len(s)] = s
            lengths[b, h] = len(s)
        if name == "edits":
            if b == 0:
                am[b, 3] = am[b, 1]                                     # the tie of the duplicate
            if b == 1:
                am[b, 7] = -np.inf
            if b == 2:                                                  # lengths outside [0, T]: clamped on the device
                store[b, 1, :T] = (hyps[1] + [int(t) for t in rng.integers(0, V - 1, size=T)])[:T]
                lengths[b, 1] = T + 7
                lengths[b, 6] = -3
    g = torch.Generator().manual_seed(900 + seed)
    prefix = torch.randn((B, P, 128), generator=g) if P else None
    return SimpleNamespace(ids=torch.from_numpy(store)[:, :n, :T], lengths=torch.from_numpy(lengths), am=torch.from_numpy(am), prefix=prefix)


def node_rows(P, nmax):
    """the product's rule for max_nodes=None: P + N is the next multiple of 8 at or above P + max_b n_nodes[b]"""
    return (P + nmax + 7) // 8 * 8 - P


def measure(name, inp):
    """float64 reference of a case -> dict; see make()"""
    V, B, n, T, P, use_eos, max_nodes, _, (aw, lw, lb) = CASES[name]
    bos = V - 1 if V < 50257 else BOS
    eos = bos if use_eos else None
    cfg = gpt_cfg(V)
    sd64, sd32 = state_dict64(V), state_dict(V)
    ids, lengths, am = inp.ids.numpy(), inp.lengths.numpy(), inp.am.numpy()
    if max_nodes is None:
        N = node_rows(P, max(RR.trie(ids[b], lengths[b], am[b], V, bos, 1 + n * T)["n_nodes"] for b in range(B)))
    else:
        N = max_nodes
    out = dict(N=N, bos=bos, eos=eos, tries=[], lm=np.zeros((B, n)), packed=np.zeros((B, n)), leak=np.zeros((B, n)), total=np.zeros((B, n)),
               order=np.zeros((B, n), dtype=np.int64), n_scored=np.zeros(B, dtype=np.int64), e32=0.0, gap=np.inf)
    for b in range(B):
        tr = RR.trie(ids[b], lengths[b], am[b], V, bos, N)
        scored = tr["leaf"] >= 0
        pf = None if inp.prefix is None else inp.prefix[b]
        lm = RR.flat_lm(sd64, cfg, ids[b], lengths[b], scored, pf, bos, eos)
        lm32 = RR.flat_lm(sd32, cfg, ids[b], lengths[b], scored, pf, bos, eos)
        out["e32"] = max(out["e32"], float(np.abs(lm32[scored] - lm[scored]).max()) if scored.any() else 0.0)
        out["packed"][b] = RR.packed_lm(sd64, cfg, tr, n, pf, eos)
        out["leak"][b] = RR.packed_lm(sd64, cfg, tr, n, pf, eos, sibling_leak=True)
        total, order, ns = RR.combine_rank(am[b], lm, RR.clamp_lengths(lengths[b], T), scored, aw, lw, lb)
        out["gap"] = min(out["gap"], RR.smallest_gap(total, scored))
        out["tries"].append(tr)
        out["lm"][b], out["total"][b], out["order"][b], out["n_scored"][b] = lm, total, order, ns
    return out


def tolerance(e32, ref):
    """the GPU test's bound on a score: max(4 e32, 8 * 2^-24 * max(1, |score|)), the rule of tests/test_ctc_beam_gpu.py"""
    return np.maximum(4.0 * e32, FLOOR * np.maximum(1.0, np.abs(np.where(np.isfinite(ref), ref, 0.0))))


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict(name, inp (generate), cfg, weights, and the float64 reference of measure()).  Cached: treat everything as read-only."""
    inp = generate(name)
    ref = measure(name, inp)
    V, B, n, T, P, use_eos, max_nodes, _, weights = CASES[name]
    if name in RANKING:
        assert ref["gap"] >= MARGIN * ref["e32"], (name, ref["gap"], ref["e32"])
        assert any(not np.array_equal(ref["order"][b], np.arange(n)) for b in range(B)), (name, ref["order"])
        fin = np.isfinite(ref["packed"])
        moved = np.abs(ref["leak"][fin] - ref["packed"][fin]).max()
        assert moved > 100.0 * tolerance(ref["e32"], ref["lm"])[fin].max(), (name, moved)
    return dict(name=name, inp=inp, cfg=gpt_cfg(V), V=V, B=B, n=n, T=T, P=P, max_nodes=max_nodes, weights=weights, **ref)
