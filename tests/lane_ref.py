"""CPU side of the token-on-the-lane kernel tests (csrc/mlp_fused.hip): the inputs of tests/test_lane_kernels_gpu.py, their float64
references, a model of the kernels' documented arithmetic (fp32 accumulation, fp32 epilogue in the kernels' evaluation order, bf16
rounding of what is stored) and the bound both are held to.  Nothing here touches a GPU: tests/test_lane_routes_cpu.py checks on these
functions alone that the model stays inside the bound and that every mix-up the kernels could commit moves the reference outside it.

Inputs follow tests/test_gemm_routes_gpu.operands (the GPU file asserts that `operands` gives the same values): integers in [-2, 2] with
an asymmetric ramp in one column of each operand, weights scaled by the power of two of `act_scale`, so every product is exact in fp32.
"""
import torch

BF = torch.bfloat16
D_MODEL, HEAD = 384, 64
W_SCALE = 2.0 ** -4                                         # test_gemm_routes_gpu.act_scale(384)
Q_SCALE = 0.1803                                            # the pre-scaled query table, as in test_gemm_routes_gpu.test_rope


def operands_cpu(M, N, Kd, seed, w_scale=1.0):
    """test_gemm_routes_gpu.operands without the upload: A [M, Kd] and W [N, Kd] (float32 values, exact in bf16), their exact float64
    product and the generator, left where `operands` leaves it"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, Kd + 8), generator=g).float()
    w = torch.randint(-2, 3, (N, Kd), generator=g).float()
    a[:, min(5, Kd - 1)] += (torch.arange(M) % 7).float()
    w[:, min(2, Kd - 1)] += (torch.arange(N) % 3).float()
    w *= w_scale
    a = a[:, :Kd].contiguous()
    assert torch.equal(a.to(BF).float(), a) and torch.equal(w.to(BF).float(), w)
    ref = a.double() @ w.double().t()
    assert float(ref.abs().max()) < 2 ** 24 * w_scale and torch.equal(ref.float().double(), ref)
    return a, w, ref, g


def bf16(x):
    return x.float().to(BF).double()


def frac(got, ref, mag, relf=2e-5):
    """largest |got - ref| / (2^-8 |ref| + 2e-5 + relf * mag): check_bound of tests/test_gemm_routes_gpu.py for bf16 outputs (relf = 2e-5)"""
    return float(((got.double() - ref).abs() / (2.0 ** -8 * ref.abs() + 2e-5 + relf * mag)).max())


def sigmoid32(x):
    """mf_sigmoid<true>: rcp(1 + exp(-x)) in fp32"""
    return 1.0 / (1.0 + torch.exp(-x))


def split13(h, M, H):
    """(a1, a3) [M, H] of an interleaved [M, 2H] (per 4 hidden units 4 columns of h1, then 4 of h3)"""
    il = h.reshape(M, H // 4, 2, 4)
    return il[:, :, 0].reshape(M, H), il[:, :, 1].reshape(M, H)


def join13(x, y):
    M, H = x.shape
    return torch.stack([x.reshape(M, H // 4, 4), y.reshape(M, H // 4, 4)], dim=2).reshape(M, 2 * H)


# ----------------------------------------------------------------------------------------------- up-projection + SwiGLU
def up_seed(M, H):
    return M + H + D_MODEL


def up_ref(acc):
    """float64 g = silu(h1) h3 of the exact interleaved product acc [M, 2H]; h13's reference is acc itself"""
    M, H = acc.shape[0], acc.shape[1] // 2
    a1, a3 = split13(acc, M, H)
    return a1 * torch.sigmoid(a1) * a3


def up_model(acc):
    """(h13, g) as the kernel documents them: the fp32 accumulator rounded to bf16; (h1 * sigmoid(h1)) * h3 in fp32, rounded"""
    M, H = acc.shape[0], acc.shape[1] // 2
    a32 = acc.float()
    a1, a3 = split13(a32, M, H)
    return bf16(a32), bf16(a1 * sigmoid32(a1) * a3)


def saturated_up_operands(M, H, values):
    """up-projection operands whose hidden units 0 .. 2 len(values) - 1 have pre-activations of exactly +v, -v for v in values, then +-1:
    activation column 9 is the constant 1 and the h1 weight rows of those units are zero except for the value in column 9.  Their h3
    rows keep the drawn weights (mixed sign and size)."""
    a, w, _, _ = operands_cpu(M, 2 * H, D_MODEL, up_seed(M, H) + 1, W_SCALE)
    a[:, 9] = 1.0
    pre = [s * float(v) for v in tuple(values) + (1,) for s in (1, -1)]
    assert len(pre) <= H
    for u, v in enumerate(pre):
        row = 8 * (u // 4) + u % 4                          # interleaved W13 row of h1 of unit u
        w[row] = 0.0
        w[row, 9] = v
    assert torch.equal(w.to(BF).float(), w)
    acc = a.double() @ w.double().t()
    assert torch.equal(acc.float().double(), acc)
    a1, _ = split13(acc, M, H)
    assert all(bool((a1[:, u] == v).all()) for u, v in enumerate(pre))
    return a, w, acc, pre


# ----------------------------------------------------------------------------------------------- q|k|v projection + RoPE
def qkv_seed(M, N):
    return M + N + D_MODEL + HEAD


def rope_tables(g, B, T, off, per_sample):
    """[2, (B,) off + T, 32, 2] float32: (cos, sin) of angles drawn per position (and per sample), and the copy scaled for the queries;
    exactly off + T rows per sample"""
    ang = torch.rand(*((B,) if per_sample else ()), off + T, HEAD // 2, generator=g) * 6.2831
    tab = torch.stack([ang.cos(), ang.sin()], -1)
    return torch.stack([tab, tab * Q_SCALE]).contiguous()


def rope_pairs(both, B, T, N, rot, qc, off, per_sample, pos_shift=0, sample_shift=0, unscaled_q=False):
    """(cos, sin) [B, T, rot / 64, 32] float32 each, as row m = b T + t must read them: table[b][off + t] of the scaled copy for the
    first qc columns, of the plain one for the rest.  pos_shift / sample_shift / unscaled_q: the mix-ups (rolled inside the table)."""
    nh, nq = rot // HEAD, qc // HEAD
    t = both.roll(-pos_shift, dims=-3)[..., off:off + T, :, :]
    if per_sample:
        t = t.roll(-sample_shift, dims=1)
    else:
        t = t[:, None].expand(2, B, T, HEAD // 2, 2)
    heads = [t[0 if unscaled_q else 1]] * nq + [t[0]] * (nh - nq)
    cs = torch.stack(heads, 2)                               # [B, T, nh, 32, 2]
    return cs[..., 0], cs[..., 1]


def qkv_ref(acc, c, s, B, T, rot):
    """float64 output [M, N] of the exact product acc rotated in its first rot columns, and the magnitude of the terms of the rotation"""
    M, N = acc.shape
    out, mag = acc.clone(), acc.abs()
    if rot:
        y = acc[:, :rot].reshape(B, T, rot // HEAD, HEAD // 2, 2)
        re, im, c, s = y[..., 0], y[..., 1], c.double(), s.double()
        out[:, :rot] = torch.stack([re * c - im * s, re * s + im * c], -1).reshape(M, rot)
        mag[:, :rot] = torch.stack([(re * c).abs() + (im * s).abs(), (re * s).abs() + (im * c).abs()], -1).reshape(M, rot)
    return out, mag


def qkv_model(acc, c, s, B, T, rot):
    """the kernel's rotation: fma(re, c, -(im * s)) and fma(re, s, im * c) in fp32 (the inner product rounded, the fma exact up to its one
    rounding), then bf16"""
    M, N = acc.shape
    out = acc.float().double()
    if rot:
        y = acc[:, :rot].float().reshape(B, T, rot // HEAD, HEAD // 2, 2)
        re, im = y[..., 0], y[..., 1]
        v0 = (re.double() * c.double() - (im * s).double()).float()
        v1 = (re.double() * s.double() + (im * c).double()).float()
        out[:, :rot] = torch.stack([v0, v1], -1).reshape(M, rot).double()
    return bf16(out)


# ----------------------------------------------------------------------------------------------- backward chain
def bwd_operands(H, rows):
    """dy [rows, 384], w2t [H, 384] (scaled), the exact dg = dy w2t^T, h13 [rows, 2H] in multiples of 1/8 with a ramp column (as
    test_gemm_routes_gpu.test_swiglu_backward), and w13t [384, 2H] with a ramp along 2H and one along d"""
    dy, w2t, dg, g = operands_cpu(rows, H, D_MODEL, H + D_MODEL + 1, W_SCALE)
    h13 = torch.randint(-24, 25, (rows, 2 * H), generator=g).float() / 8
    h13[:, 3] += (torch.arange(rows) % 5).float() / 4
    w13t = torch.randint(-2, 3, (D_MODEL, 2 * H), generator=g).float()
    w13t[2, :] += (torch.arange(2 * H) % 5).float()
    w13t[:, 1] += (torch.arange(D_MODEL) % 3).float()
    w13t /= 16
    assert torch.equal(h13.to(BF).float(), h13) and torch.equal(w13t.to(BF).float(), w13t)
    return dy, w2t, dg, h13, w13t


def saturated_bwd_operands(H, rows, values):
    """bwd_operands with the h1 columns of hidden units 0 .. 2 len(values) + 1 set to exactly +v, -v for v in values, then +-1"""
    dy, w2t, dg, h13, w13t = bwd_operands(H, rows)
    pre = [s * float(v) for v in tuple(values) + (1,) for s in (1, -1)]
    for u, v in enumerate(pre):
        h13[:, 8 * (u // 4) + u % 4] = v
    assert torch.equal(h13.to(BF).float(), h13)
    return dy, w2t, dg, h13, w13t, pre


def bwd_ref(dg, h13):
    """float64 dh13 [M, 2H] (interleaved) and its magnitude: dh1 = dg sg a3 (1 + a1 (1 - sg)), dh3 = dg sg a1; mag = |dg sg a3| (1 + |a1|), |dh3|"""
    M, H = dg.shape
    a1, a3 = split13(h13.double(), M, H)
    sg = torch.sigmoid(a1)
    d1, d3 = dg * sg * a3 * (1 + a1 * (1 - sg)), dg * sg * a1
    return join13(d1, d3), join13((dg * sg * a3).abs() * (1 + a1.abs()), d3.abs())


def bwd_model(dg, h13):
    """dswiglu_piece in fp32: ds = g * sg; (ds * a3) * (1 + a1 * (1 - sg)) and ds * a1, rounded to bf16"""
    M, H = dg.shape
    a1, a3 = split13(h13.float(), M, H)
    g = dg.float()
    sg = sigmoid32(a1)
    ds = g * sg
    return bf16(join13(ds * a3 * (1.0 + a1 * (1.0 - sg)), ds * a1))


def dx_ref(dh, w13t):
    """dx [M, 384] in float64 from the dh13 the kernel stored (dh13 is held to float64 on its own), the magnitude |dh13| |w13t|^T and
    the relative factor of the bound: the worst case of an fp32 sum of 2H terms, at least the project's 2e-5"""
    dh, w = dh.double(), w13t.double()
    return dh @ w.t(), dh.abs() @ w.abs().t(), max(2e-5, dh.shape[1] * 2.0 ** -24)


def dx_model(dh, w13t):
    return bf16(dh.float() @ w13t.float().t())
