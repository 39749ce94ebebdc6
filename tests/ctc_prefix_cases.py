"""The cases of the CTC prefix scorer's tests, shared by tests/test_ctc_prefix_cpu.py and tests/test_ctc_prefix_gpu.py: their inputs and
what the restatement (tests/ctc_prefix_ref.py) expects, computed once per process.

ONE_STEP: one launch of fk_ctc_prefix_score from planted states.  The planted states are fp32 values (what the kernel reads), so the
float64 oracle and the float32 restatement start from the same numbers and differ by the arithmetic of the one step only.
LOOPS: a whole search without a model (flat attention rows, planted CTC logits), composed with the select restatements of the beam tests."""
import functools
from collections import namedtuple

import numpy as np

from tests import ctc_prefix_ref as R
from tests.sample_ref import philox4x32_10
from tests.test_eos_cpu import eos_step_ref, lenpow_table

f32, f64 = np.float32, np.float64


def bf16_round(x):
    """fp32 values rounded to the nearest bfloat16 (ties to even), still stored as fp32"""
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(f32).reshape(np.shape(x))


# ------------------------------------------------------------------------------------------------ one step from planted states
# S, W, k, T, C, dtype, step (0: nothing advances; odd / even: both parities of the ping-pong), broadcast, extra columns behind C in a
# frame (padded ldt), input_lengths (None: T each), eos (-1: none; then some rows are finished), weight
One = namedtuple("One", "S W k T C dtype step broadcast pad lengths eos weight")
ONE_STEP = [
    One(1, 1, 1, 1, 3, "f32", 0, False, 0, None, -1, 0.3),
    One(1, 1, 1, 2, 41, "bf16", 1, False, 0, None, -1, 0.5),
    One(1, 1, 1, 1024, 3, "f32", 2, False, 0, None, -1, 1.0),
    One(1, 4, 20, 1, 41, "bf16", 1, False, 3, None, 7, 0.3),
    One(1, 4, 20, 2, 41, "f32", 2, False, 0, (2,), 7, 0.5),
    One(1, 4, 20, 33, 41, "f32", 1, False, 7, None, 7, 0.3),
    One(1, 4, 20, 33, 3, "f32", 3, False, 0, (20,), 1, 0.7),
    One(1, 4, 20, 4, 50258, "f32", 1, False, 0, None, 50256, 0.3),
    One(1, 4, 20, 4, 50258, "bf16", 2, False, 6, (3,), 50256, 0.3),
    One(3, 4, 20, 33, 41, "f32", 2, False, 0, (0, 33, 17), 7, 0.5),
    One(3, 4, 20, 33, 41, "bf16", 1, False, 7, (33, 0, 5), 7, 0.3),
    One(3, 4, 20, 33, 41, "f32", 0, True, 0, (33, 12, 0), 7, 0.3),
    One(3, 4, 20, 1024, 41, "f32", 1, False, 0, (1024, 700, 0), 7, 0.3),
    One(3, 4, 20, 2, 3, "f32", 1, False, 1, None, -1, 0.3),
    One(2, 16, 64, 33, 41, "f32", 1, False, 0, (33, 0), 7, 0.3),
    One(2, 16, 64, 1024, 41, "bf16", 2, False, 0, (1000, 1024), 7, 0.5),
    One(2, 16, 64, 2, 3, "f32", 2, False, 0, None, -1, 0.3),
    One(2, 16, 64, 1, 41, "f32", 1, False, 5, (1, 0), 7, 0.3),
]


def one_id(c):
    return "S{}W{}k{}-T{}-C{}-{}-step{}{}{}{}".format(c.S, c.W, c.k, c.T, c.C, c.dtype, c.step, "-bcast" if c.broadcast else "",
                                                      "-ldt+%d" % c.pad if c.pad else "", "-len" if c.lengths else "")


def _ulp32(x):
    return float(np.spacing(f32(max(abs(float(x)), 1e-30))))


@functools.lru_cache(maxsize=None)
def one_step(c):
    """-> dict: the inputs (numpy), `want` float64 joint values, `floor` mask, `want32` the float32 restatement (exact for floor entries
    and untouched rows), `tol`, `err32`, the expected new states (float64 / float32) and which rows hold one"""
    rng = np.random.default_rng([c.S, c.W, c.k, c.T, c.C, c.step, c.pad, len(c.dtype)])
    S, W, k, T, C = c.S, c.W, c.k, c.T, c.C
    R_ = S * W
    blank = C - 1 if C > 3 else 1
    scale = 3.0 if T <= 64 else 1.0
    logits = (rng.standard_normal((S, T, C)) * scale).astype(f32)
    if c.dtype == "bf16":
        logits = bf16_round(logits)
    lens = [T] * S if c.lengths is None else list(c.lengths)
    labels = [x for x in range(C) if x != blank and x != c.eos]
    ys = {dt: [R.log_softmax_rows(logits[g, :lens[g]], dt) for g in range(S)] for dt in (f64, f32)}
    advance = c.step > 0 and not c.broadcast
    fin = np.zeros(R_, np.int32)
    if c.eos >= 0 and W > 1 and not c.broadcast:
        fin[rng.integers(0, W, S) + W * np.arange(S)] = 1
    # the planted hypotheses: 0 .. 3 labels each, one in three with a repeated label; their fp32 states are the inputs
    old32, plant = [], []
    for g in range(S):
        hs = []
        for b in range(W):
            n = min(int(rng.integers(0, 4)), max(lens[g] - 1, 0) // 2) if not (c.step == 0 and b == 0) else 0     # what the frames can spell
            seq = [int(rng.choice(labels)) for _ in range(n)]
            if n >= 2 and rng.integers(0, 3) == 0:
                seq[-1] = seq[-2]
            hs.append(R.hyp_of(ys[f64][g], blank, seq))
        h = R.Hyps.cat(hs)
        old32.append(R.Hyps(h.r_n.astype(f32), h.r_b.astype(f32), h.psi.astype(f32), h.last))
        plant.append(h)
    parent = rng.integers(-1, W + 1, R_).astype(np.int32)                       # with entries outside [0, W): clamped
    tok = rng.choice(labels, R_).astype(np.int64)
    for r in range(0, R_, 3):                                                   # every third row repeats its parent's last label
        p = int(np.clip(parent[r], 0, W - 1))
        last = int(old32[r // W].last[p])
        if last >= 0:
            tok[r] = last
    if R_ >= 8:
        tok[5], tok[6] = C + 2, blank                                           # two impossible hypotheses: every candidate meets the floor
    new = {}
    for dt in (f64, f32):
        out = []
        for g in range(S):
            h = R.Hyps(old32[g].r_n.astype(dt), old32[g].r_b.astype(dt), old32[g].psi.astype(dt), old32[g].last)
            if advance:
                sl = slice(g * W, g * W + W)
                h = R.extend(ys[dt][g], blank, h.take(np.clip(parent[sl], 0, W - 1)), tok[sl])
            out.append(h)
        new[dt] = out
    rows = S if c.broadcast else R_
    top_lp = (-rng.random((rows, k)) * 6 - 0.01).astype(f32)
    top_id = np.empty((rows, k), np.int64)
    for q in range(rows):
        pool = np.arange(-1, C + 2) if C <= k else np.concatenate([rng.choice(C, k, replace=False), [-1, C, C + 1]])
        top_id[q] = rng.choice(pool, k, replace=C <= k)
        g, b = (q, 0) if c.broadcast else divmod(q, W)
        special = [int(new[f64][g].last[b]), blank, C + int(rng.integers(0, 3)), c.eos if c.eos >= 0 else labels[0]]
        if k >= 4:
            top_id[q, rng.choice(k, 4, replace=False)] = special
        else:                                                                   # k < 4: one label that can follow
            top_id[q, 0] = next(x for x in labels if x != special[0])
    want, floor = R.score_rows(ys[f64], blank, new[f64], top_lp, top_id, c.weight, c.eos, fin, W, c.broadcast)
    want32, floor32 = R.score_rows(ys[f32], blank, new[f32], top_lp, top_id, c.weight, c.eos, fin, W, c.broadcast)
    assert np.array_equal(floor, floor32)
    psi_all = np.concatenate([h.psi for h in new[f64]])
    with np.errstate(invalid="ignore"):
        cand = [(want[q] - (1 - f64(f32(c.weight))) * top_lp[q]) for q in range(rows)]
    psi_max = max([0.0] + [abs(x) for x in psi_all if np.isfinite(x)])
    if c.weight > 0:                                                            # psi' = psi + delta of every scored candidate
        for q in range(rows):
            g, b = (q, 0) if c.broadcast else divmod(q, W)
            p = new[f64][g].psi[b]
            if np.isfinite(p) and not fin[g * W + b]:
                d = cand[q][~floor[q]] / f64(f32(c.weight))
                psi_max = max([psi_max] + list(np.abs(p + d)))
    err32 = float(np.abs(want32.astype(f64) - want)[~floor].max()) if (~floor).any() else 0.0
    tol = max(4 * err32, _ulp32(psi_max))
    live = np.array([not fin[r] for r in range(R_)])
    return dict(case=c, blank=blank, logits=logits, lens=lens, fin=fin, old=old32, parent=parent, tok=tok, top_lp=top_lp, top_id=top_id,
                want=want, want32=want32, floor=floor, err32=err32, tol=tol, psi_max=psi_max, new=new[f64], new32=new[f32], advance=advance,
                live=live, plant=plant)


# ------------------------------------------------------------------------------------------------ a whole search without a model
Loop = namedtuple("Loop", "T W k C weight target")
LOOPS = [Loop(8, 4, 8, 41, 0.5, (5, 9, 9, 3)), Loop(40, 4, 8, 41, 0.5, (5, 9, 9, 3, 3, 17))]
# Salts of the noise and of the candidate lists, chosen on the CPU from the float64 restatement's own decision margins (the first salt that
# keeps every margin >= 1e-3; tests/test_ctc_prefix_cpu.py asserts it), before any kernel ran.
LOOP_SALT = {8: 0, 40: 1}
LOOP_EOS, LOOP_SEED, PEAK = 38, 0x0123_4567_89AB_CDEF, 8.0


def gumbel_draws(top_lp, broadcast, W, seed, step):
    """the draws of fk_beam_select* for one sentence: picks[i] = beam i's entries by draw rank, margins[i] = the gap between its W-th and
    (W+1)-th Gumbel key"""
    k = top_lp.shape[1]
    picks, margins = [], []
    for i in range(W):
        row = top_lp[0 if broadcast else i]
        keys = np.empty(k, f32)
        for j in range(k):
            c0 = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (step & 0xFFFFFFFF, step >> 32, i, 0xBEA30000 | j))[0]
            u = (f32(c0 >> 8) + f32(0.5)) * f32(1.0 / 16777216.0)
            keys[j] = row[j] - np.log(-np.log(u, dtype=f32), dtype=f32)
        order = sorted(range(k), key=lambda j: (-keys[j], j))
        margins.append(float(keys[order[W - 1]] - keys[order[W]]) if k > W else np.inf)
        picks.append(order[:W])
    return picks, margins


def loop_logits(c, salt):
    """[T, C] fp32: the frames spell the target (a blank between repeated labels, blanks behind it), the spelled class PEAK above noise"""
    rng = np.random.default_rng([c.T, salt, 77])
    blank = c.C - 1
    path = []
    for i, lab in enumerate(c.target):
        if i and c.target[i - 1] == lab:
            path.append(blank)
        path.append(lab)
    rep = max(1, (c.T - 2) // len(path))
    frames = [x for x in path for _ in range(rep)]
    frames += [blank] * (c.T - len(frames))
    lg = (rng.standard_normal((c.T, c.C)) * 0.5).astype(f32)
    lg[np.arange(c.T), frames] += f32(PEAK)
    return lg


@functools.lru_cache(maxsize=None)
def loop(c, salt=None):
    """The float64 restatement of the whole search (one sentence): per step the candidate lists, the joint values, the select's decisions
    and the states.  -> dict with `steps` (list of dicts) and `margin`, the smallest decision margin."""
    salt = LOOP_SALT[c.T] if salt is None else salt
    rng = np.random.default_rng([c.T, salt, 78])
    W, k, C, blank = c.W, c.k, c.C, c.C - 1
    logits = loop_logits(c, salt)
    y = {dt: R.log_softmax_rows(logits, dt) for dt in (f64, f32)}
    table = lenpow_table(len(c.target) + 4, 0.0)
    n_steps = len(c.target) + 2
    labels = [x for x in range(C) if x not in (blank, LOOP_EOS)]
    hyp = {dt: R.empty(y[dt], blank, W) for dt in (f64, f32)}
    scores, lens, fin = np.zeros(W, f32), np.zeros(W, np.int32), np.zeros(W, np.int32)
    seqs = [[] for _ in range(W)]
    steps, margin = [], np.inf
    for s in range(n_steps):
        bc = s == 0
        rows = 1 if bc else W
        top_id = np.empty((rows, k), np.int64)
        for q in range(rows):
            planted = c.target[len(seqs[q])] if len(seqs[q]) < len(c.target) else LOOP_EOS
            others = [x for x in labels if x != planted]
            top_id[q] = rng.choice(others, k, replace=False)
            top_id[q, rng.integers(0, k)] = planted
        top_lp = np.full((rows, k), -np.log(k), f32)
        want, floor = R.score_rows([y[f64]], blank, [hyp[f64]], top_lp, top_id, c.weight, LOOP_EOS, fin, W, bc)
        want32, _ = R.score_rows([y[f32]], blank, [hyp[f32]], top_lp, top_id, c.weight, LOOP_EOS, fin, W, bc)
        jt = want.astype(f32)
        picks, key_margins = gumbel_draws(jt, bc, W, LOOP_SEED, s)
        margin = min([margin] + [m for m, f in zip(key_margins, fin) if not f])
        if floor[[q for q in range(rows) if not fin[q]]].any():
            margin = 0.0                                                         # floor entries tie at fp32's spacing near 5e9: not a case
        parent, cur, new_scores, new_lens, new_fin, cands = eos_step_ref(jt, top_id, bc, W, picks, scores, lens, fin, LOOP_EOS, table)
        # a candidate is the sequence it leads to: one proposed twice ties exactly on both sides, distinct ones must lie apart
        what = lambda cd: tuple(seqs[cd[5]]) + (() if fin[cd[5]] else (cd[4],))
        margin = min([margin] + [float(a[0] - b[0]) for a, b in zip(cands[:W], cands[1:W + 1]) if what(a) != what(b)])
        steps.append(dict(top_lp=top_lp, top_id=top_id, want=want, want32=want32, floor=floor, fin_in=fin.copy(), parent=list(parent), cur=list(cur),
                          scores=new_scores.copy(), fin=np.array(new_fin, np.int32), hyp=hyp[f64], hyp32=hyp[f32]))
        seqs = [seqs[p] + ([t] if not fin[p] else []) for p, t in zip(parent, cur)]
        for dt in (f64, f32):
            hyp[dt] = R.extend(y[dt], blank, hyp[dt].take(parent), np.array(cur))
        scores, lens, fin = new_scores, np.array(new_lens, np.int32), np.array(new_fin, np.int32)
    return dict(case=c, logits=logits, blank=blank, steps=steps, margin=margin, table=table, final_scores=scores, final_seqs=seqs, final_fin=fin,
                final_lens=lens)
