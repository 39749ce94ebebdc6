"""float64 restatement (numpy) of the per-session input adapter of csrc/dayadapt.hip: the forward in fk_patchify's layout with its zero
padding and its one rounding, and both gradients from a d_tok in the same layout.

    d = day[b];  y[b, t, :] = x[b, t, :] + x[b, t, :] @ delta[d] + bias[d]   if 0 <= d < n_days, else y[b, t, :] = x[b, t, :]
    tok[b, (t // P) * C + c, p] = y[b, (t // P) * P + p, c] for p < P, 0 for P <= p < ldp
    d_delta[d, c, c'] = sum_{b: day[b] = d} sum_t x[b, t, c] dy[b, t, c'],   d_bias[d, c'] = sum_{b: day[b] = d} sum_t dy[b, t, c']
    with dy[b, tp * P + p, c'] = d_tok[b, tp * C + c', p]

`defect` plants one bookkeeping mistake (tests/test_day_adapter_cpu.py shows that each breaks the bound on a named case)."""
import numpy as np

DEFECTS = ("delta_transposed", "first_day_for_all", "bias_dropped", "day_clamped", "pc_swapped", "absent_unwritten")


def valid_days(day, B, n_days):
    """(index array int64 [B], mask bool [B]): day None = nothing valid"""
    if day is None:
        return np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
    d = np.asarray(day, dtype=np.int64)
    ok = (d >= 0) & (d < n_days)
    return np.where(ok, d, 0), ok


def adapt(x, day, delta, bias, defect=None):
    """y [B, T, C] float64"""
    x = np.asarray(x, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    bias = np.asarray(bias, dtype=np.float64)
    B = x.shape[0]
    n_days = delta.shape[0]
    if day is not None and defect == "first_day_for_all":
        day = np.full(B, np.asarray(day)[0])
    if day is not None and defect == "day_clamped":
        day = np.clip(np.asarray(day), 0, n_days - 1)
    d, ok = valid_days(day, B, n_days)
    dl = delta[d]
    if defect == "delta_transposed":
        dl = dl.transpose(0, 2, 1)
    y = x + np.einsum("btc,bcd->btd", x, dl)
    if defect != "bias_dropped":
        y = y + bias[d][:, None, :]
    return np.where(ok[:, None, None], y, x)


def patchify(y, P, ldp):
    """[B, T, C] -> [B, (T / P) * C, ldp], columns P.. zero"""
    B, T, C = y.shape
    nT = T // P
    tok = np.zeros((B, nT * C, ldp), dtype=y.dtype)
    tok[:, :, :P] = y.reshape(B, nT, P, C).transpose(0, 1, 3, 2).reshape(B, nT * C, P)
    return tok


def unpatchify(tok, T, C, P, defect=None):
    """[B, (T / P) * C, ldp] -> dy [B, T, C] (the padding columns are not read)"""
    B = tok.shape[0]
    nT = T // P
    if defect == "pc_swapped":                # the token row read as (p, c) instead of (c, p)
        flat = np.ascontiguousarray(tok[:, :, :P]).reshape(B, nT, C * P)
        return flat.reshape(B, nT, P, C).reshape(B, T, C)
    return tok[:, :, :P].reshape(B, nT, C, P).transpose(0, 1, 3, 2).reshape(B, T, C)


def round_to(v, dtype):
    """float64 values rounded once to 'fp32' or 'bf16' (round to nearest even), returned as float64"""
    v = np.asarray(v, dtype=np.float64)
    if dtype == "fp32":
        return v.astype(np.float32).astype(np.float64)
    # bf16: 8 significant bits, ONE rounding from the float64 value (a cast through fp32 would round twice)
    a = np.abs(v)
    q = 2.0 ** (np.floor(np.log2(np.maximum(a, np.finfo(np.float32).tiny))) - 7)
    return np.where(a > 0, np.rint(v / q) * q, 0.0)


def forward(x, day, delta, bias, P, ldp, dtype=None, defect=None):
    """tok [B, (T / P) * C, ldp] float64; dtype 'fp32' / 'bf16' applies the final rounding, None leaves the exact values"""
    tok = patchify(adapt(x, day, delta, bias, defect), P, ldp)
    return tok if dtype is None else round_to(tok, dtype)


def backward(x, day, d_tok, P, n_days, defect=None, prefill=None):
    """(d_delta [n_days, C, C], d_bias [n_days, C]) float64.  prefill: what the output buffers held before (only the
    'absent_unwritten' defect lets it through)"""
    x = np.asarray(x, dtype=np.float64)
    B, T, C = x.shape
    dy = unpatchify(np.asarray(d_tok, dtype=np.float64), T, C, P, defect)
    if day is not None and defect == "first_day_for_all":
        day = np.full(B, np.asarray(day)[0])
    if day is not None and defect == "day_clamped":
        day = np.clip(np.asarray(day), 0, n_days - 1)
    d, ok = valid_days(day, B, n_days)
    d_delta = np.zeros((n_days, C, C))
    d_bias = np.zeros((n_days, C))
    if defect == "absent_unwritten" and prefill is not None:
        d_delta[:] = prefill
        d_bias[:] = prefill
    seen = set()
    for b in range(B):
        if not ok[b]:
            continue
        g = x[b].T @ dy[b]
        if defect == "delta_transposed":
            g = g.T
        if defect == "absent_unwritten" and prefill is not None and int(d[b]) not in seen:
            d_delta[d[b]] = 0.0
            d_bias[d[b]] = 0.0
        seen.add(int(d[b]))
        d_delta[d[b]] += g
        if defect != "bias_dropped":
            d_bias[d[b]] += dy[b].sum(0)
    return d_delta, d_bias


def half_ulp(ref, dtype):
    """half a unit in the last place of `dtype` at |ref| (float64 array): the error of one rounding to nearest"""
    bits = 24 if dtype == "fp32" else 8
    a = np.abs(ref)
    e = np.floor(np.log2(np.maximum(a, np.finfo(np.float32).tiny)))
    return np.where(a > 0, 2.0 ** (e - bits), 0.0)


def torch_composition(x, day, delta, bias, d_tok, P, ldp, dtype):
    """The same forward and gradients composed from torch ops on the CPU in `dtype` (torch.float64: must equal the restatement;
    torch.float32: its distance from the float64 values is the yardstick of the kernels' bound).  Returns numpy float64
    (tok, d_delta, d_bias)."""
    import torch
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    dl = torch.tensor(np.asarray(delta), dtype=dtype, requires_grad=True)
    bs = torch.tensor(np.asarray(bias), dtype=dtype, requires_grad=True)
    g = torch.tensor(np.asarray(d_tok), dtype=dtype)
    B, T, C = xt.shape
    idx, ok = valid_days(day, B, dl.shape[0])
    idx, ok = torch.from_numpy(idx), torch.from_numpy(ok)
    y = xt + torch.einsum("btc,bcd->btd", xt, dl[idx]) + bs[idx][:, None, :]
    y = torch.where(ok[:, None, None], y, xt)
    nT = T // P
    tok = torch.nn.functional.pad(y.view(B, nT, P, C).permute(0, 1, 3, 2).reshape(B, nT * C, P), (0, ldp - P))
    (tok * g).sum().backward()
    return tok.detach().double().numpy(), dl.grad.double().numpy(), bs.grad.double().numpy()


def bounds(x, day, delta, bias, d_tok, P, ldp):
    """The float64 reference (exact tok, d_delta, d_bias) and the scalar yardsticks 4 * max |torch fp32 composition - reference| of
    the three tensors: the project's usual bound for an fp32 kernel (the forward adds half_ulp() for its one rounding)."""
    import torch
    ref = (forward(x, day, delta, bias, P, ldp), *backward(x, day, d_tok, P, np.asarray(delta).shape[0]))
    t32 = torch_composition(x, day, delta, bias, d_tok, P, ldp, torch.float32)
    return ref, tuple(4.0 * float(np.max(np.abs(a - r))) for a, r in zip(t32, ref))
