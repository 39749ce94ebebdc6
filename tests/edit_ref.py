"""Python-int / float64 restatement of csrc/editdist.hip (semantics: include/franken_hip.h, "edit distance"), independent of the kernels:
the textbook Levenshtein table, the pairwise table of an n-best list, the MBR posterior / risk / ranking (in float64, and in float32 with
the kernel's operation order for the rounding yardstick e32), and the MWER loss as torch's own F.ctc_loss on log_softmax plus the combine,
under autograd."""
import numpy as np
import torch
import torch.nn.functional as F


def distance(a, b):
    """unit-cost Levenshtein distance of two sequences: the full (len(a) + 1) x (len(b) + 1) table"""
    a, b = [int(t) for t in a], [int(t) for t in b]
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
    return D[len(a)][len(b)]


def seq(row, length, pad_value):
    """the sequence a row holds: its first `length` entries (clamped into [0, len(row)]), or with length None those before the first pad_value"""
    row = [int(t) for t in row]
    if length is None:
        return row[:row.index(pad_value)] if pad_value in row else row
    return row[:min(max(int(length), 0), len(row))]


def distances(a, alen, b, blen, pad_value):
    """a [B, n_a, La] (n_a = n or 1), b [B, n, Lb] (array-likes), lengths arrays or None -> (dist int64 [B, n], measured lengths of a [B, n_a])"""
    B, n = len(b), len(b[0])
    n_a = len(a[0])
    out = np.zeros((B, n), dtype=np.int64)
    la = np.zeros((B, n_a), dtype=np.int64)
    for g in range(B):
        for h in range(n):
            ha = 0 if n_a == 1 else h
            x = seq(a[g][ha], None if alen is None else alen[g][ha], pad_value)
            y = seq(b[g][h], None if blen is None else blen[g][h], pad_value)
            out[g, h] = distance(x, y)
            la[g, ha] = len(x)
    return out, la


def pairwise(ids, lengths, scores):
    """one sentence: ids [n, T], lengths [n], scores [n] or None -> int64 [n, n]; -1 in the row and column of a non-finite score"""
    n = len(ids)
    ok = [True] * n if scores is None else [bool(np.isfinite(s)) for s in scores]
    out = -np.ones((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            if ok[i] and ok[j]:
                out[i, j] = 0 if i == j else distance(seq(ids[i], lengths[i], None), seq(ids[j], lengths[j], None))
    return out


def mbr(dist, scores, scale, dtype=np.float64):
    """one sentence -> (risk [n] in input order (+inf: invalid), order [n], n_valid); every operation in `dtype`, sums in ascending j over
    the valid j, one rounding per operation"""
    f = dtype
    n = len(scores)
    ok = [bool(np.isfinite(s)) for s in scores]
    valid = [j for j in range(n) if ok[j]]
    risk = np.full(n, np.inf, dtype=f)
    if valid:
        t = {j: f(f(scale) * f(scores[j])) for j in valid}
        m = max(t.values())
        w = {j: f(np.exp(f(t[j] - m))) for j in valid}
        Z = f(0.0)
        for j in valid:
            Z = f(Z + w[j])
        for i in valid:
            r = f(0.0)
            for j in valid:
                r = f(r + f(f(w[j] / Z) * f(dist[i][j])))
            risk[i] = r
    order = sorted(valid, key=lambda i: (risk[i], i)) + [i for i in range(n) if not ok[i]]
    return risk, np.array(order, dtype=np.int64), len(valid)


def smallest_gap(risk, n_valid_mask):
    """the smallest non-zero difference between two valid risks (inf when there is none)"""
    r = np.sort(np.asarray(risk, dtype=np.float64)[n_valid_mask])
    d = np.diff(r)
    d = d[d > 0]
    return float(d.min()) if d.size else np.inf


def mwer_combine(nll, errors, valid):
    """one sentence, torch: nll a [n] tensor or a list of n 0-d tensors (any float dtype, may carry a graph; entries of invalid hypotheses
    are not touched), errors [n] ints, valid [n] bools, at least one of them set -> loss (0-d tensor).  p = softmax(-nll) over the valid
    ones, loss = sum p (e - mean e)."""
    idx = [i for i in range(len(valid)) if valid[i]]
    z = -torch.stack([nll[i] for i in idx])
    p = torch.softmax(z, dim=0)
    e = torch.tensor([float(errors[i]) for i in idx], dtype=z.dtype)
    return (p * (e - e.mean())).sum()


def mwer(logits, targets, target_lengths, ids, lengths, scores, blank, ce_weight=0.0, dtype=torch.float64, max_len=255):
    """logits [B, T, C] (torch, any float dtype; evaluated in `dtype` on the CPU), targets int64 [B, L] with target_lengths [B], the list
    ids [B, n, Th] / lengths [B, n] / scores [B, n] -> (loss float, dlogits [B, T, C] in `dtype`, nll [B, n] numpy (inf: infeasible), errors
    [B, n], valid bool [B, n]).  nll is F.ctc_loss on log_softmax per hypothesis; the result is the mean of the sentences' terms over the
    sentences that have a valid hypothesis (+ ce_weight * the mean-reduced CTC loss of the targets)."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    B, T, C = x.shape
    n = ids.shape[1]
    lp = F.log_softmax(x, dim=2).transpose(0, 1)                        # [T, B, C]
    nll_np = np.full((B, n), np.inf)
    errors = np.zeros((B, n), dtype=np.int64)
    valid = np.zeros((B, n), dtype=bool)
    terms, have = [], 0
    for b in range(B):
        ref = seq(targets[b].tolist(), target_lengths[b], None)
        row = []
        for i in range(n):
            hyp = seq(ids[b, i].tolist(), lengths[b, i], None)
            errors[b, i] = distance(ref, hyp)
            ok = bool(np.isfinite(float(scores[b, i]))) and len(hyp) <= max_len
            v = None
            if ok:
                tg = torch.tensor([hyp + [blank + 1] * (1 if not hyp else 0)], dtype=torch.int64)
                v = F.ctc_loss(lp[:, b:b + 1], tg, torch.tensor([T]), torch.tensor([len(hyp)]), blank=blank, reduction="sum", zero_infinity=False)
                nll_np[b, i] = float(v.detach())
                ok = bool(np.isfinite(nll_np[b, i]))
            valid[b, i] = ok
            row.append(v)
        if valid[b].any():
            have += 1
            terms.append(mwer_combine(row, errors[b], valid[b]))
    loss = x.new_zeros(()) if not terms else torch.stack(terms).sum() / have
    if ce_weight:
        tl = torch.tensor([len(seq(targets[b].tolist(), target_lengths[b], None)) for b in range(B)])
        loss = loss + ce_weight * F.ctc_loss(lp, targets.clamp(min=0), torch.full((B,), T), tl, blank=blank, reduction="mean", zero_infinity=False)
    if loss.requires_grad:
        loss.backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return float(loss.detach()), grad.detach(), nll_np, errors, valid

