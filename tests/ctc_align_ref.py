"""Numpy restatement of the CTC forced alignment (fk_ctc_align: include/franken_hip.h holds the specification, csrc/ctc.hip the kernel), and
the inputs tests/test_ctc_align_cpu.py and tests/test_ctc_align_gpu.py share.

viterbi() is the definition in float64; with dtype=np.float32 the same recursion runs in float32 (row_lse included), which is what the
tolerances of the GPU tests are measured from.  brute_force() enumerates every alignment of a tiny sample and is what pins viterbi().

Per sample: T_b clamped into [0, T], L_b into [0, Lmax] (without target_lengths: the leading entries that differ from pad_value), labels
clamped into [0, C) and off the blank (a label equal to the blank becomes blank - 1, or 1 when the blank is 0), lp = log_softmax(logits),
l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L_b + 1.
  v_0(0) = lp_0(blank), v_0(1) = lp_0(l_1), else -inf;  v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if s odd and l'_s != l'_{s-2}) + lp_t(l'_s)
  exact ties: the smaller move (stay before s-1 before s-2); the end state is the better of S-1 and S-2, S-1 on an exact tie.
A sample without alignment (score -inf): path all pad, index all -1, start = end = -1, label_lp = 0.  T_b = 0 = L_b: score 0, empty rows."""
import functools

import numpy as np
import torch

from tests import ctc_cases as CC
from tests import ctc_ref as R

NEG = -np.inf
PACK, CHUNK = 16, 256                                  # csrc/ctc.hip: CTC_ALIGN_PACK, CTC_ALIGN_CHUNK (kernels.py mirrors them)


def clamp_inputs(targets, T, C, input_lengths=None, target_lengths=None, blank=0, pad_value=-100):
    """-> (T_b [B], L_b [B], labels [B, Lmax] clamped as the kernels clamp them)"""
    tg = np.asarray(targets, dtype=np.int64)
    B, Lmax = tg.shape
    Tb = np.full(B, T, dtype=np.int64) if input_lengths is None else np.clip(np.asarray(input_lengths, dtype=np.int64), 0, T)
    Lb = R.lengths_from_padding(tg, pad_value) if target_lengths is None else np.clip(np.asarray(target_lengths, dtype=np.int64), 0, Lmax)
    lab = np.clip(tg, 0, C - 1)
    lab[lab == blank] = 1 if blank == 0 else blank - 1
    return Tb, Lb, lab


def log_softmax(logits, dtype):
    x = np.asarray(logits).astype(dtype)
    m = x.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype)).astype(dtype)
    return (x - lse).astype(dtype), lse[..., 0]


def best_path(lp, ext):
    """lp [T_b >= 1, C] log-probabilities in the working dtype, ext the extended labels -> (score, states [T_b]) or (-inf, None)"""
    Tn, S = lp.shape[0], len(ext)
    dt = lp.dtype
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    e = lp[:, ext]
    v = np.full(S, NEG, dtype=dt)
    v[:2] = e[0, :2]
    back = np.zeros((Tn, S), dtype=np.int8)
    pad2 = np.full(2, NEG, dtype=dt)
    for t in range(1, Tn):
        p = np.concatenate([pad2, v])
        n1, n2 = p[1:-1], np.where(skip, p[:-2], NEG).astype(dt)
        best, code = v.copy(), np.zeros(S, dtype=np.int8)
        m1 = n1 > best
        best[m1], code[m1] = n1[m1], 1
        m2 = n2 > best
        best[m2], code[m2] = n2[m2], 2
        v = (best + e[t]).astype(dt)
        back[t] = code
    s = S - 2 if S >= 2 and v[S - 2] > v[S - 1] else S - 1
    score = v[s]
    if score == NEG:
        return NEG, None
    states = np.zeros(Tn, dtype=np.int64)
    for t in range(Tn - 1, -1, -1):
        states[t] = s
        s -= int(back[t, s])
    return float(score), states


def outputs_of(states, ext, lp, T, Lmax, pad, dtype):
    """one sample's rows from its state sequence (None: no alignment)"""
    path, index = np.full(T, pad, dtype=np.int64), np.full(T, -1, dtype=np.int64)
    start, end = np.full(Lmax, -1, dtype=np.int64), np.full(Lmax, -1, dtype=np.int64)
    label_lp = np.zeros(Lmax, dtype=dtype)
    if states is not None:
        n = len(states)
        path[:n] = ext[states]
        index[:n] = np.where(states % 2 == 1, states // 2, -1)
        for t, s in enumerate(states):
            if s % 2 == 1:
                i = s // 2
                if start[i] < 0:
                    start[i] = t
                end[i] = t + 1
                label_lp[i] = label_lp[i] + lp[t, ext[s]]          # ascending frames, one add a frame in the working dtype
    return path, index, start, end, label_lp


def viterbi(logits, targets, input_lengths=None, target_lengths=None, blank=0, pad_value=-100, pad=-100, dtype=np.float64):
    """logits [B, T, C], targets int [B, Lmax] -> dict(score [B], path [B, T], index [B, T], start / end [B, Lmax], label_lp [B, Lmax],
    states: per sample the state sequence or None, Tb, Lb, labels (clamped), lp [B, T, C], lse [B, T])"""
    x = np.asarray(logits)
    B, T, C = x.shape
    Lmax = np.asarray(targets).shape[1]
    Tb, Lb, lab = clamp_inputs(targets, T, C, input_lengths, target_lengths, blank, pad_value)
    lp, lse = log_softmax(x, dtype)
    out = dict(score=np.zeros(B, dtype=dtype), path=np.zeros((B, T), dtype=np.int64), index=np.zeros((B, T), dtype=np.int64),
               start=np.zeros((B, Lmax), dtype=np.int64), end=np.zeros((B, Lmax), dtype=np.int64), label_lp=np.zeros((B, Lmax), dtype=dtype),
               states=[], Tb=Tb, Lb=Lb, labels=lab, lp=lp, lse=lse)
    for b in range(B):
        ext = R.extended(lab[b, :Lb[b]], blank)
        tb = int(Tb[b])
        if tb == 0:
            score, states = (0.0, np.zeros(0, dtype=np.int64)) if Lb[b] == 0 else (NEG, None)
        else:
            score, states = best_path(lp[b, :tb], ext)
        out["score"][b] = score
        out["states"].append(states)
        out["path"][b], out["index"][b], out["start"][b], out["end"][b], out["label_lp"][b] = outputs_of(states, ext, lp[b], T, Lmax, pad, dtype)
    return out


def alignments(Tn, ext):
    """every state sequence of Tn >= 1 frames over the extended labels ext that CTC admits"""
    S = len(ext)
    out = []

    def grow(seq):
        if len(seq) == Tn:
            if seq[-1] >= S - 2:
                out.append(tuple(seq))
            return
        s = seq[-1]
        for m in (0, 1, 2):
            n = s + m
            if n >= S or (m == 2 and not (n % 2 == 1 and ext[n] != ext[n - 2])):
                continue
            grow(seq + [n])

    for s0 in range(min(2, S)):
        grow([s0])
    return out


def brute_force(lp, ext):
    """the best alignment by enumeration: the score of a sequence is the sum of its lp in frame order (what the recursion forms); among
    sequences of exactly equal score the tie rules pick the one that is largest read from the last frame to the first (the larger end
    state; then, frame by frame backwards, the smaller move) -> (score, states) or (-inf, None)"""
    best, arg = NEG, None
    for seq in alignments(lp.shape[0], ext):
        v = lp[0, ext[seq[0]]]
        for t in range(1, len(seq)):
            v = v + lp[t, ext[seq[t]]]
        if v > best or (v == best and v > NEG and seq[::-1] > arg[::-1]):
            best, arg = v, seq
    return (float(best), np.array(arg, dtype=np.int64)) if best > NEG else (NEG, None)


def path_score(lp, path, tb):
    """the float64 score of a class sequence: the sum of lp_t(path_t) in frame order"""
    v = 0.0
    for t in range(tb):
        v = v + lp[t, path[t]]
    return v


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def random_alignment(rng, tb, ext):
    """a uniformly drawn set of visited states and frame counts: a valid alignment of tb frames, as states [tb]"""
    S = len(ext)
    must = [s % 2 == 1 or (0 < s < S - 1 and ext[s - 1] == ext[s + 1]) for s in range(S)]
    optional = [s for s in range(S) if not must[s]]
    room = tb - sum(must)
    assert room >= 0
    take = set(rng.choice(optional, size=int(rng.integers(0, min(room, len(optional)) + 1)), replace=False).tolist()) if optional else set()
    visited = [s for s in range(S) if must[s] or s in take]
    if not visited:                                       # the empty target: S = 1 and its blank is optional, but a frame needs a state
        visited = [0]
    cuts = np.sort(rng.choice(np.arange(1, tb), size=len(visited) - 1, replace=False)) if len(visited) > 1 else np.zeros(0, dtype=np.int64)
    counts = np.diff(np.concatenate([[0], cuts, [tb]])).astype(np.int64)
    return np.repeat(np.array(visited, dtype=np.int64), counts)


def with_stride(x, ld):
    B, T, C = x.shape
    store = torch.full((B, T, ld), float("nan"))
    store[:, :, :C] = x
    return store[:, :, :C]


@functools.lru_cache(maxsize=None)
def edge_case(Lmax):
    """T_b in {1, PACK - 1, PACK, PACK + 1, CHUNK - 1, CHUNK, CHUNK + 1} at S = 2 Lmax + 1 (Lmax 2: the wave route, 32: the LDS route), the
    blank in the middle of the classes, a padded row stride; L_b = min(Lmax, (T_b + 1) / 2), so that every sample has an alignment"""
    Tb = [1, PACK - 1, PACK, PACK + 1, CHUNK - 1, CHUNK, CHUNK + 1]
    B, T, C = len(Tb), CHUNK + 1, 9 if Lmax <= 2 else 40
    blank = C // 2
    rng = np.random.default_rng(900 + Lmax)
    Lb = [min(Lmax, (t + 1) // 2) for t in Tb]
    targets = torch.full((B, Lmax), CC.PAD, dtype=torch.int64)
    for b in range(B):
        labels = CC._labels(rng, Lmax, C, blank)
        assert Tb[b] >= Lb[b] + CC.repeats(labels[:Lb[b]])
        targets[b, :Lb[b]] = torch.tensor(labels[:Lb[b]], dtype=torch.int64)
    g = torch.Generator().manual_seed(77 + Lmax)
    logits = with_stride(3.0 * torch.randn((B, T, C), generator=g), C + 3)
    return dict(name=f"edge{2 * Lmax + 1}", logits=logits, targets=targets, input_lengths=torch.tensor(Tb, dtype=torch.int64),
                target_lengths=torch.tensor(Lb, dtype=torch.int64), blank=blank, infeasible=0, ld=C + 3)


NAMES = list(CC.CASES) + ["edge5", "edge65"]


def case(name):
    return edge_case({"edge5": 2, "edge65": 32}[name]) if name.startswith("edge") else CC.make(name)


@functools.lru_cache(maxsize=None)
def planted(name):
    """The twin of a case: the same shapes, lengths and targets; logits uniform in [-1, 1] plus 8 at the class of a randomly drawn valid
    alignment.  Any other alignment loses at least 6 per frame at which it differs (before and after bf16 rounding, which moves a logit by
    at most 2^-8 relative), and an alignment is determined by its classes: the planted one is the unique optimum by a margin no fp32 error
    reaches.  -> the case dict with `planted`: the states per sample (None where the sample has no alignment)."""
    c = dict(case(name))
    B, T, C = c["logits"].shape
    rng = np.random.default_rng(4242 + sum(map(ord, name)))
    x = rng.uniform(-1.0, 1.0, size=(B, T, C)).astype(np.float32)
    Tb, Lb, lab = clamp_inputs(c["targets"].numpy(), T, C, c["input_lengths"].numpy(), c["target_lengths"].numpy(), c["blank"])
    states = []
    for b in range(B):
        ext = R.extended(lab[b, :Lb[b]], c["blank"])
        tb = int(Tb[b])
        if tb < Lb[b] + CC.repeats(lab[b, :Lb[b]]) or tb == 0:
            states.append(None)
            continue
        st = random_alignment(rng, tb, ext)
        x[b, np.arange(tb), ext[st]] += 8.0
        states.append(st)
    c["logits"] = with_stride(torch.from_numpy(x), c["ld"])
    c["planted"] = states
    c["name"] = name + "_planted"
    return c
