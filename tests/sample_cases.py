"""The table of sampler cases shared by tests/test_sample_draws_cpu.py and tests/test_sample_draws_gpu.py: the smallest shapes at which
each mechanism of sample_topk_kernel can fail.

    V       1; 37 (one partial wave); 1000 (chunk 1, 24 idle threads); 1024; 1025 (chunk 2, 511 idle threads, thread 512 with one element);
            50257 (chunk 50, thread 1005 cut to 7 elements, 18 idle)
    top_k   off; 1; 8 on integer-valued logits (several entries tie with the 8th: more than 8 stay); 40; V - 1; >= V
    T       1.0, 0.7, 1.3
    top_p   1.0; 0.45 and 0.70 on placed-mass rows, whose nucleus margin is >= MIN_MARGIN (sample_ref.kept asserts it)
    seed    below 2^32; with a non-zero high word
    step    0; 1; 2^32 + 5
    rows    B = 257 DIFFERENT rows per launch (one more than 8 bits of row index); one case has B = 1

Row kinds: `normal` is standard normal times `scale`; `integer` is round(2 * normal), so values repeat; `placed` puts six heavy tokens (.97
of the mass) on index 0, V - 1, both sides of chunk, wave and half-block boundaries, over a light jittered tail, every row shifted by its
own constant so that the keys change sign and exponent from row to row.  `ninf` rows hold a few -inf entries, the last index among them.

Untruncated rows of the whole vocabulary are scaled by 4: at scale 2 about a fifth of 50257 tokens hold more than 2 EPS of the mass each,
their boundaries alone would make > 5 % of the draws ambiguous, and an ambiguous draw checks less than an exact one."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from tests import sample_ref as R

SEED_LO = 20240611
SEED_HI = 0x1234_5678_9ABC_DEF0          # non-zero high word, positive as the int64 the state holds
STEP_BIG = 2 ** 32 + 5
HEADS = (0.30, 0.22, 0.14, 0.12, 0.10, 0.09)          # mass_gt: 0 .30 .52 .66 .78 .88 | .97; behind top_k = 5, of .88: 0 .341 .591 .75 .886
LAUNCHES = 2                             # consecutive steps a case is drawn at: step, step + 1


@dataclass(frozen=True)
class Case:
    name: str
    V: int
    kind: str                            # normal | integer | placed
    top_k: Optional[int]
    T: float
    top_p: float = 1.0
    seed: int = SEED_LO
    step: int = 0
    scale: float = 2.0
    ninf: bool = False
    B: int = 257


CASES = [
    Case("v1", 1, "normal", None, 1.0),
    Case("v37-normal", 37, "normal", None, 1.0, seed=SEED_HI, step=1),
    Case("v37-ties-k8", 37, "integer", 8, 0.7),
    Case("v37-placed-kV-1", 37, "placed", 36, 1.3),
    Case("v1000-normal", 1000, "normal", None, 1.0),
    Case("v1000-x4-k40", 1000, "normal", 40, 0.7, seed=SEED_HI, scale=4.0),
    Case("v1000-ties-k8", 1000, "integer", 8, 1.0, step=1),
    Case("v1000-placed-p45", 1000, "placed", None, 0.7, top_p=0.45),
    Case("v1000-placed-k5-p70", 1000, "placed", 5, 1.0, top_p=0.70, seed=SEED_HI),
    Case("v1000-ninf", 1000, "normal", None, 1.3, ninf=True),
    Case("v1000-k1", 1000, "normal", 1, 1.0),
    Case("v1000-b1-k40", 1000, "normal", 40, 1.0, B=1),
    Case("v1024-normal-bigstep", 1024, "normal", None, 1.0, step=STEP_BIG),
    Case("v1024-placed-k40", 1024, "placed", 40, 1.0),
    Case("v1024-x4-kV+5", 1024, "normal", 1029, 1.3, scale=4.0),
    Case("v1025-normal", 1025, "normal", None, 1.0, seed=SEED_HI),
    Case("v1025-placed", 1025, "placed", None, 0.7),
    Case("v1025-ninf-kV-1", 1025, "normal", 1024, 1.0, ninf=True, step=1),
    Case("v1025-placed-p70", 1025, "placed", None, 1.3, top_p=0.70),
    Case("v50257-x4", 50257, "normal", None, 1.0, scale=4.0),
    Case("v50257-k40-bigstep", 50257, "normal", 40, 0.7, seed=SEED_HI, step=STEP_BIG),
    Case("v50257-placed", 50257, "placed", None, 1.0, step=1),
    Case("v50257-placed-k40", 50257, "placed", 40, 1.3),
    Case("v50257-placed-p45", 50257, "placed", None, 0.7, top_p=0.45, seed=SEED_HI),
    Case("v50257-ninf-kV-1", 50257, "normal", 50256, 1.0, scale=4.0, ninf=True),
    Case("v50257-ties-k8", 50257, "integer", 8, 1.0),
    Case("v50257-kV", 50257, "normal", 50257, 0.7, scale=4.0, seed=SEED_HI),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def special_positions(V):
    """index 0 and V - 1, both sides of the first two chunk boundaries, of a wave's and of the half block's, both sides of the boundary of the
    thread that V cuts short, and three spots in between"""
    c = R.chunk_of(V)
    cut = (V // c) * c
    spots = [0, V - 1, c - 1, c, 2 * c - 1, 2 * c, 64 * c - 1, 64 * c, 512 * c - 1, 512 * c, cut - 1, cut, V // 3 + 1, V // 2, 2 * V // 3]
    return sorted({s for s in spots if 0 <= s < V})


def _placed(rng, B, V, T):
    spots = special_positions(V)
    assert len(spots) >= len(HEADS) and V > len(HEADS)
    tail = np.log((1.0 - sum(HEADS)) / (V - len(HEADS)))
    rows = np.empty((B, V), np.float32)
    for b in range(B):
        pos = ([V - 1] if b % 4 != 3 else []) + ([0] if b % 3 == 0 else [])
        rest = [s for s in spots if s not in pos]
        pos += [int(s) for s in rng.permutation(rest)[:len(HEADS) - len(pos)]]
        logp = tail + 0.5 * rng.standard_normal(V)
        logp[pos] = np.log(rng.permutation(HEADS))
        rows[b] = (T * (logp + rng.uniform(-6.0, 6.0))).astype(np.float32)          # logits * (1 / T) is log p + the row's shift again
    return rows


def logits_of(case):
    """fp32 [B, V], the same on every machine: seeded by the case's place in the table"""
    rng = np.random.default_rng(7000 + CASES.index(case))
    B, V = case.B, case.V
    if case.kind == "normal":
        rows = (rng.standard_normal((B, V)) * case.scale).astype(np.float32)
    elif case.kind == "integer":
        rows = np.round(rng.standard_normal((B, V)) * 2.0).astype(np.float32) + 0.0          # + 0.0: no negative zero, whose key differs from +0's
    else:
        rows = _placed(rng, B, V, case.T)
    if case.ninf:
        for b in range(B):
            rows[b, rng.choice(V - 1, 3, replace=False)] = -np.inf
        rows[:, V - 1] = -np.inf
    return rows


def refs_of(case, rows, top_p=None):
    """RowRef per row at the case's parameters (top_p: the case's, or the one given)"""
    p = case.top_p if top_p is None else top_p
    return [R.row_ref(r, case.T, case.top_k, p) for r in rows]


def uniforms_of(case, launch=0, seed=None, step=None):
    """u of every row at the case's step + launch"""
    seed = case.seed if seed is None else seed
    step = case.step if step is None else step
    return [R.uniform(seed, step + launch, b) for b in range(case.B)]
