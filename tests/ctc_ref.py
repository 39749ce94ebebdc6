"""Float64 numpy restatement of the CTC path (csrc/ctc.hip): row_lse, alpha, beta, nll, d-logits and the greedy collapse.

Semantics: F.ctc_loss(log_softmax(logits, -1).transpose(0, 1), targets, input_lengths, target_lengths, blank, reduction, zero_infinity);
tests/test_ctc_cpu.py pins this file to torch's float64 CPU implementation.  alpha and beta both include the frame's own
log-probability, so alpha_t(s) + beta_t(s) - lp_t(l'_s) sums to -nll at every frame."""
import numpy as np

NEG = -np.inf


def logsumexp(a, axis=None):
    a = np.asarray(a, dtype=np.float64)
    m = np.max(a, axis=axis, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        r = np.log(np.sum(np.exp(a - m0), axis=axis, keepdims=True)) + m0
    return r.reshape(()).item() if axis is None else np.squeeze(r, axis=axis)


def lengths_from_padding(targets, pad_value=-100):
    """number of leading entries that differ from pad_value, per row"""
    out = []
    for row in np.asarray(targets):
        hit = np.nonzero(row == pad_value)[0]
        out.append(int(hit[0]) if len(hit) else len(row))
    return np.array(out, dtype=np.int64)


def extended(labels, blank):
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    return ext


def row_lse(logits):
    return logsumexp(np.asarray(logits, dtype=np.float64), axis=-1)


def lattice(lp, ext):
    """lp float64 [T, C] log-probabilities of one sample's frames, ext its extended labels -> (alpha, beta) [T, S]"""
    T, S = lp.shape[0], len(ext)
    skip = np.zeros(S, dtype=bool)                    # s - 2 -> s is allowed: a label that differs from the label before it
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    alpha = np.full((T, S), NEG)
    beta = np.full((T, S), NEG)
    e = lp[:, ext]                                    # [T, S] the frame's log-probability of every state's class
    pad2 = np.full(2, NEG)
    alpha[0, :2] = e[0, :2]
    for t in range(1, T):
        p = np.concatenate([pad2, alpha[t - 1]])      # p[s + 2] = alpha[t - 1, s]
        alpha[t] = logsumexp(np.stack([p[2:], p[1:-1], np.where(skip, p[:-2], NEG)]), axis=0) + e[t]
    beta[T - 1, -2:] = e[T - 1, -2:]
    skip_up = np.concatenate([skip, [False, False]])[2:]   # s -> s + 2 is allowed
    for t in range(T - 2, -1, -1):
        p = np.concatenate([beta[t + 1], pad2])
        beta[t] = logsumexp(np.stack([p[:-2], p[1:-1], np.where(skip_up, p[2:], NEG)]), axis=0) + e[t]
    return alpha, beta


def ctc(logits, targets, input_lengths=None, target_lengths=None, blank=0, pad_value=-100, zero_infinity=False, want_lattice=False):
    """logits [B, T, C], targets int [B, Lmax] -> dict: nll [B] (after zero_infinity), raw [B], unit [B, T, C] = d nll_b / d logits
    (zero rows past T_b; zero for a sample without alignment under zero_infinity, NaN without), T_b, L_b and, on request, the per-sample
    (alpha, beta) lattices."""
    x = np.asarray(logits, dtype=np.float64)
    B, T, C = x.shape
    tg = np.asarray(targets)
    Tb = np.full(B, T, dtype=np.int64) if input_lengths is None else np.asarray(input_lengths, dtype=np.int64)
    Lb = lengths_from_padding(tg, pad_value) if target_lengths is None else np.asarray(target_lengths, dtype=np.int64)
    lse = row_lse(x)
    lp = x - lse[..., None]
    raw = np.zeros(B)
    unit = np.zeros((B, T, C))
    lats = []
    for b in range(B):
        ext = extended(tg[b, :Lb[b]], blank)
        tb = int(Tb[b])
        if tb == 0:
            raw[b] = 0.0 if Lb[b] == 0 else np.inf
            lats.append(None)
            continue
        alpha, beta = lattice(lp[b, :tb], ext)
        lats.append((alpha, beta))
        raw[b] = -logsumexp(alpha[tb - 1, -2:])
        if not np.isfinite(raw[b]):
            unit[b, :tb] = 0.0 if zero_infinity else np.nan
            continue
        ab = alpha + beta
        unit[b, :tb] = np.exp(lp[b, :tb])
        for c in np.unique(ext):                      # occupancy of class c at every frame: the states that carry it
            unit[b, :tb, c] -= np.exp(logsumexp(ab[:, ext == c], axis=1) + raw[b] - lp[b, :tb, c])
    nll = np.where(np.isinf(raw), 0.0, raw) if zero_infinity else raw.copy()
    out = dict(nll=nll, raw=raw, unit=unit, Tb=Tb, Lb=Lb, lse=lse, lp=lp)
    if want_lattice:
        out["lattice"] = lats
    return out


def reduce(nll, Lb, reduction):
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    return (nll / np.maximum(Lb, 1)).mean()


def dlogits(ref, reduction, gout):
    """gradient of sum(gout * reduce(nll)) for the dict ctc() returned; gout: scalar for 'sum' / 'mean', [B] for 'none'"""
    B = len(ref["nll"])
    g = np.broadcast_to(np.asarray(gout, dtype=np.float64), (B,)).copy()
    if reduction == "mean":
        g = g / (B * np.maximum(ref["Lb"], 1))
    return ref["unit"] * g[:, None, None]


def collapse(argmax, input_lengths=None, blank=0, pad=-100):
    """[B, T] frame labels -> (ids [B, T] padded with pad, lengths [B]): repeated frames merged, blanks dropped"""
    a = np.asarray(argmax)
    B, T = a.shape
    ids = np.full((B, T), pad, dtype=np.int64)
    lens = np.zeros(B, dtype=np.int64)
    for b in range(B):
        tb = T if input_lengths is None else int(input_lengths[b])
        prev, out = None, []
        for t in range(tb):
            if a[b, t] != blank and a[b, t] != prev:
                out.append(a[b, t])
            prev = a[b, t]
        ids[b, :len(out)] = out
        lens[b] = len(out)
    return ids, lens
