"""The CTC cases tests/test_ctc_cpu.py and tests/test_ctc_gpu.py share: the smallest shapes at which each mechanism of csrc/ctc.hip can
fail.  Logits are 3 * randn, targets contain adjacent repeats, sample 0 has the full lengths, the others T_b in [T / 2, T] and L_b in
[0, Lmax] (hand-picked where a case needs a particular sample).  Every case carries the number of samples without any alignment
(T_b < L_b + adjacent repeats) it is expected to contain; make() asserts it, so a drifting generator cannot turn a case into the trivial
one unnoticed."""
import functools

import numpy as np
import torch

PAD = -100

#        B,   T,     C, Lmax, blank, row stride, infeasible samples
CASES = {
    "a":   (4,  12,     5,   4,     0,   5, 0),     # wave route; L = 0; one sample with a single alignment
    "b31": (3,  80,   300,  31,   299, 304, 0),     # S = 63: the last wave-route size; C no multiple of the vector width, padded rows
    "b32": (3,  80,   300,  32,   299, 320, 0),     # S = 65: the first LDS-route size
    "c":   (2, 600,    41, 255,     0,  41, 0),     # S = 511, the top of the envelope; nll ~ 3e3
    "d":   (4,  32, 50258,  25, 50257, 50258, 2),   # the project's vocabulary; two sentences that do not fit
    "e":   (2,  16,     6,   6,     0,   6, 0),     # one class in six states
}


def repeats(labels):
    labels = list(labels)
    return sum(1 for i in range(1, len(labels)) if labels[i] == labels[i - 1])


def _labels(rng, n, C, blank):
    """n labels off the blank, about every fifth a copy of the one before it"""
    out = []
    for i in range(n):
        if i and rng.random() < 0.2:
            out.append(out[-1])
        else:
            v = int(rng.integers(C - 1))
            out.append(v + 1 if v >= blank else v)
    return out


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict(logits fp32 [B, T, C] (a view into [B, T, row stride] storage), targets int64 [B, Lmax] padded with -100, input_lengths,
    target_lengths, blank, infeasible).  Cached: treat the tensors as read-only."""
    B, T, C, Lmax, blank, ld, infeasible = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    Tb = [T] + [int(rng.integers(T // 2, T + 1)) for _ in range(B - 1)]
    Lb = [Lmax] + [int(rng.integers(0, Lmax + 1)) for _ in range(B - 1)]
    labels = [_labels(rng, Lmax, C, blank) for _ in range(B)]
    if name == "a":
        labels = [[1, 1, 2, 3], [4, 2, 1, 3], [2, 2, 3, 3], [4, 1, 1, 2]]
        Tb, Lb = [12, 7, 6, 9], [4, 0, 4, 3]           # sample 1: empty target; sample 2: T_b = L_b + repeats, one alignment: 2 _ 2 3 _ 3
    if name == "c":
        Tb[1] = int(rng.integers(520, T + 1))
    if name == "d":
        labels = [[int(v) for v in rng.choice(C - 1, Lmax, replace=False)] for _ in range(B)]   # the blank is the last class
        labels[0][7], labels[0][15] = labels[0][6], labels[0][14]
        labels[1][3], labels[2][4] = labels[1][2], labels[2][3]
        labels[3][5], labels[3][9] = labels[3][4], labels[3][8]
        Tb, Lb = [32, 16, 24, 20], [25, 20, 10, 19]    # samples 1 (20 labels in 16 frames) and 3 (19 labels + repeats in 20) do not fit
    if name == "e":
        labels = [[3] * 6, [2] * 6]
        Tb, Lb = [16, 12], [6, 6]
    targets = torch.full((B, Lmax), PAD, dtype=torch.int64)
    for b in range(B):
        targets[b, :Lb[b]] = torch.tensor(labels[b][:Lb[b]], dtype=torch.int64)
    n_inf = sum(1 for b in range(B) if Tb[b] < Lb[b] + repeats(labels[b][:Lb[b]]))
    assert n_inf == infeasible, (name, n_inf, infeasible)
    assert any(repeats(labels[b][:Lb[b]]) for b in range(B)), name
    g = torch.Generator().manual_seed(1234 + sum(map(ord, name)))
    store = torch.full((B, T, ld), float("nan"))
    store[:, :, :C] = 3.0 * torch.randn((B, T, C), generator=g)
    return dict(name=name, logits=store[:, :, :C], targets=targets, input_lengths=torch.tensor(Tb, dtype=torch.int64),
                target_lengths=torch.tensor(Lb, dtype=torch.int64), blank=blank, infeasible=infeasible, ld=ld)


def torch_ctc(case, dtype, reduction="none", zero_infinity=False, logits=None):
    """torch's CPU F.ctc_loss in `dtype` on the case (logits: a replacement for the case's own, e.g. bf16-rounded) -> (loss, d loss.sum()
    / d logits), both in `dtype`"""
    import torch.nn.functional as F
    x = (case["logits"] if logits is None else logits).detach().to(dtype).contiguous().requires_grad_(True)
    lp = F.log_softmax(x, dim=-1).transpose(0, 1)
    tg = case["targets"].clamp(min=0)
    loss = F.ctc_loss(lp, tg, case["input_lengths"], case["target_lengths"], blank=case["blank"], reduction=reduction, zero_infinity=zero_infinity)
    loss.sum().backward()
    return loss.detach(), x.grad
