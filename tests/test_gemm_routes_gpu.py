"""Every kernel fk_gemm_nt chooses between (csrc/gemm.hip's NtRoute) under every epilogue it runs there, and the small fk_gemm_tn kernel
with its slab reduction, against a float64 reference on the CPU.

Before it launches, every test asks the host-side route query (kernels.gemm_nt_route / gemm_tn_route) which kernel its shape reaches and
compares that with the route its id names: a changed threshold fails the test instead of silently turning it into a second copy of
another one (tests/test_gemm_routes_cpu.py pins the same table without a GPU; the shapes live in tests/cases.py).

Operands are small integers with an asymmetric ramp in one column of each (any fragment / tile / row mix-up is a hard mismatch), A is a
view with row stride K + 8, and every product is exact in fp32 (|ref| < 2^24 is asserted).  So
  * plain / bias / residual outputs must be BIT-EQUAL to the float64 reference (fp32 output) or to its single rounding (bf16 output);
  * for the non-linear epilogues one operand is scaled by a power of two (pre-activations of a few units, still exact).  The linear
    parts of their outputs (h13, the unrotated columns) are bit-equal again.  The rest is held to
        |got - ref| <= [2^-8 |ref|, bf16 outputs only] + 2e-5 + 2e-5 * mag
    one bf16 ulp of the reference for the one rounding of the output, plus the project's fp32 tolerance (atol = rtol = 2e-5 of
    test_kernels_gpu.close) with the relative part applied to the magnitude of the terms that enter the last subtraction / product:
    mag = |re cos| + |im sin| for RoPE, |dg sg a3| (1 + |a1|) for dh1 of the SwiGLU backward, |ref| otherwise — so cancellation does
    not turn into a relative-error failure.  Every element is compared.
  * rows are independent and the epilogue is one body of code: a call on >= 4096 rows (ring kernels, NT_BIG) or on more than 256 tiles
    (NT_GLDS) must be torch.equal to the same call on row pieces that take the short-latency 128 x 128 kernel.
Each fused test prints "FRAC <epilogue> <route> <largest error / bound>".

What reaches what (ids start with the route; "F32" = fp32 operands on the staged kernel):
  test_plain_bias_residual_exact   all seven routes and F32; NT_GLDS with 288 tiles (one per workgroup), 575 = 23 x 25 and 1125 tiles (the
                                   `tile += nbx` loop, a tile count 8 does not divide), N % 128 != 0, and N % 8 != 0 (scalar sweep over
                                   clamped B rows); NT_BIG at M = 4096 + 72, N = 256 and 512; res_rows 1 / 5 / 24 through the residual
                                   prefetch of NT_RING192 / NT_RING128 and the in-sweep form of the others
  test_swiglu_forward / _backward  NT_RING2, NT_RING128, NT_BIG, NT_GLDS, NT_GLDS4, NT_STAGED, F32 (the backward's h13 prefetch on the
                                   ring kernels)
  test_rope                        the same routes; D 8 / 16 / 64 / 128, T 5 / 57 / 300, bias, pos_off, pre-scaled query columns, shared and
                                   per-sample tables (the wrap at a sample boundary in the prefetched and the in-sweep form)
  test_gemm_tn_exact               one split, empty trailing splits, a 3-row last split, the scalar slab reduction, the large-tile kernel
(the token-on-the-lane kernels that take over from 45 825 rows on at K = 384: tests/test_lane_kernels_gpu.py, on these operands and this
bound; their per-sample table also in tests/test_kernels_gpu.py, test_qkv_projection_with_rope_token_on_the_lane_...)"""
import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SENTINEL = -7.0


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def cid(c):
    return "-".join(str(x) for x in c)


def threshold(monkeypatch, ring_min):
    if ring_min is None:
        monkeypatch.delenv("FK_NT_RING_MIN_TILES", raising=False)
    else:
        monkeypatch.setenv("FK_NT_RING_MIN_TILES", ring_min)


def route_name(K, M, N, Kd, dtype, vec_epi=True, mode=0, has_rope=False):
    return K.NT_ROUTE_NAMES[K.gemm_nt_route(M, N, Kd, dtype, vec_epi, mode, has_rope)]


def reaches(K, route, M, N, Kd, dtype, vec_epi=True, mode=0, has_rope=False):
    got = route_name(K, M, N, Kd, dtype, vec_epi, mode, has_rope)
    assert got == ("NT_STAGED_F32" if route == "F32" else route), f"{M} x {N} x {Kd} reaches {got}, not {route}"


def vec_epi(N, out=None, res=None):
    """what launch_nt decides: 8 columns per lane need N, ldc (, ldr) % 8 == 0 and 16-byte aligned C (, residual); out=None: a fresh [M, N]"""
    ok = N % 8 == 0 and (out is None or (out.stride(0) % 8 == 0 and out.data_ptr() % 16 == 0))
    return ok and (res is None or (res.stride(0) % 8 == 0 and res.data_ptr() % 16 == 0))


def operands(M, N, Kd, dtype, seed, w_scale=1.0):
    """A [M, Kd] as a view with row stride Kd + 8 and W [N, Kd] on the GPU, and their exact float64 product"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, Kd + 8), generator=g).float()
    w = torch.randint(-2, 3, (N, Kd), generator=g).float()
    a[:, min(5, Kd - 1)] += (torch.arange(M) % 7).float()
    w[:, min(2, Kd - 1)] += (torch.arange(N) % 3).float()
    w *= w_scale
    ad, wd = a.to(dtype).cuda()[:, :Kd], w.to(dtype).cuda()
    assert torch.equal(ad.float().cpu(), a[:, :Kd]) and torch.equal(wd.float().cpu(), w)         # representable in the compute dtype
    ref = a[:, :Kd].double() @ w.double().t()
    assert float(ref.abs().max()) < 2 ** 24 * w_scale and torch.equal(ref.float().double(), ref)
    return ad, wd, ref, g


def act_scale(Kd):
    """W scale of the non-linear cases: sums of Kd products of integers in [-2, 2] have a deviation of 2 sqrt(Kd), i.e. 2 .. 2.5 after it"""
    return 2.0 ** -3 if Kd <= 128 else 2.0 ** -4


def rounded(ref, dtype):
    """the float64 reference in the output dtype: one rounding (ref is representable in fp32 wherever this is used for equality)"""
    return ref.float() if dtype == F32 else ref.float().to(BF).float()


def guarded_view(M, N, dtype, pad):
    """an [M, N] view `pad` columns into a sentinel-filled [M, N + 2 pad] buffer (allocated through the guard-band allocator)"""
    buf = torch.zeros(M, N + 2 * pad, dtype=dtype, device="cuda")
    buf.fill_(SENTINEL)
    return buf, buf[:, pad:pad + N]


def neighbours_untouched(buf, N, pad):
    b = buf.float().cpu()
    return bool((b[:, :pad] == SENTINEL).all()) and bool((b[:, pad + N:] == SENTINEL).all())


def strided(t, dtype, pad):
    """t [R, N] on the GPU as a view of an [R, N + pad] buffer"""
    full = torch.zeros(t.shape[0], t.shape[1] + pad)
    full[:, :t.shape[1]] = t
    return full.to(dtype).cuda()[:, :t.shape[1]]


def check_bound(tag, route, got, ref, mag, dtype):
    """|got - ref| <= [2^-8 |ref|] + 2e-5 + 2e-5 mag on every element (see the module docstring); prints the largest fraction of the bound"""
    got, bound = got.double().cpu(), 2e-5 + 2e-5 * mag + (2.0 ** -8 * ref.abs() if dtype == BF else 0.0)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    frac = ((got - ref).abs() / bound)
    worst = float(frac.max())
    print(f"FRAC {tag} {route} {worst:.4f}")
    if worst > 1.0:
        idx = [int(i) for i in np.unravel_index(int(frac.argmax()), tuple(frac.shape))]
        raise AssertionError(f"{tag} on {route}: error {worst:.3f} x its bound at {idx}: got {float(got[tuple(idx)])!r}, want {float(ref[tuple(idx)])!r}; "
                             f"{int((frac > 1).sum())} elements over")


# ----------------------------------------------------------------------------------------------- plain / bias / residual
@pytest.mark.parametrize("case", cases.NT_PLAIN_CASES, ids=cid)
def test_plain_bias_residual_exact(K, monkeypatch, case):
    """fp32 output bit-equal to the float64 reference, bf16 output to its single rounding, on every route: no epilogue, bias + strided
    residual into a strided out= view (columns beside it untouched), periodic residual with res_rows = 1, 5 and 24 (fewer than the 8
    rows of a prefetch step, not a divisor of 8, and the space-embedding case) — ragged last row tile everywhere."""
    route, M, N, Kd, ring_min = case
    threshold(monkeypatch, ring_min)
    dtype = F32 if route == "F32" else BF
    ad, wd, ref, g = operands(M, N, Kd, dtype, seed=M + N + Kd)
    vec = N % 8 == 0
    pad = 8 if vec else 3
    outs = [F32] if dtype == F32 else [F32, BF]
    for odt in outs:
        reaches(K, route, M, N, Kd, dtype, vec_epi(N))
        assert torch.equal(K.gemm_nt(ad, wd, out_dtype=odt).float().cpu(), rounded(ref, odt)), f"plain, {odt}"
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    res = torch.randint(-4, 5, (M, N), generator=g).float()
    resd = strided(res, dtype, pad)
    for odt in outs:
        buf, view = guarded_view(M, N, odt, pad)
        assert vec_epi(N, view, resd) == vec
        reaches(K, route, M, N, Kd, dtype, vec)
        K.gemm_nt(ad, wd, bias=bias.to(dtype).cuda(), residual=resd, out_dtype=odt, out=view)
        assert torch.equal(view.float().cpu(), rounded(ref + bias.double() + res.double(), odt)), f"bias + residual, {odt}"
        assert neighbours_untouched(buf, N, pad)
    for i, rr in enumerate((1, 5, 24)):
        tab = torch.randint(-4, 5, (rr, N), generator=g).float()
        tabd = strided(tab, dtype, pad)
        odt = outs[i % len(outs)]
        want = ref + tab.double()[torch.arange(M) % rr]
        reaches(K, route, M, N, Kd, dtype, vec_epi(N, None, tabd))
        got = K.gemm_nt(ad, wd, residual=tabd, res_rows=rr, out_dtype=odt)
        assert torch.equal(got.float().cpu(), rounded(want, odt)), f"res_rows {rr}, {odt}"
        odt = outs[(i + 1) % len(outs)]
        buf, view = guarded_view(M, N, odt, pad)
        reaches(K, route, M, N, Kd, dtype, vec_epi(N, view, tabd))
        K.gemm_nt(ad, wd, bias=bias.to(dtype).cuda(), residual=tabd, res_rows=rr, out_dtype=odt, out=view)
        assert torch.equal(view.float().cpu(), rounded(want + bias.double(), odt)), f"bias + res_rows {rr} into a view, {odt}"
        assert neighbours_untouched(buf, N, pad)


# ----------------------------------------------------------------------------------------------- fused epilogues
def pieces(M, step=1000):
    return [(lo, min(M, lo + step)) for lo in range(0, M, step)]


def wants_pieces(route):
    return route in ("NT_RING2", "NT_RING128", "NT_BIG", "NT_GLDS")


@pytest.mark.parametrize("case", cases.NT_SWIGLU_CASES, ids=cid)
def test_swiglu_forward(K, monkeypatch, case):
    """h13 = A W13^T in the interleaved layout (per 4 hidden units 4 columns of h1, then 4 of h3): bit-equal to the exact product rounded
    once; g = silu(h1) h3 from the unrounded accumulator within the bound of the module docstring (mag = |g|)."""
    route, M, H, Kd, ring_min = case
    threshold(monkeypatch, ring_min)
    dtype = F32 if route == "F32" else BF
    ad, w13, acc, _ = operands(M, 2 * H, Kd, dtype, seed=M + H + Kd, w_scale=act_scale(Kd))
    reaches(K, route, M, 2 * H, Kd, dtype, mode=1)
    h13, g = K.gemm_nt_swiglu(ad, w13)
    if wants_pieces(route):
        for lo, hi in pieces(M):
            reaches(K, "NT_GLDS4", hi - lo, 2 * H, Kd, dtype, mode=1)
            h, g2 = K.gemm_nt_swiglu(ad[lo:hi], w13)
            assert torch.equal(h13[lo:hi], h) and torch.equal(g[lo:hi], g2), f"rows {lo}..{hi} differ from the 128 x 128 kernel's"
    assert torch.equal(h13.float().cpu(), rounded(acc, dtype))
    il = acc.view(M, H // 4, 2, 4)
    a1, a3 = il[:, :, 0].reshape(M, H), il[:, :, 1].reshape(M, H)
    ref = a1 * torch.sigmoid(a1) * a3
    check_bound("swiglu_fwd", route, g, ref, ref.abs(), dtype)


@pytest.mark.parametrize("case", cases.NT_DSWIGLU_CASES, ids=cid)
def test_swiglu_backward(K, monkeypatch, case):
    """dh13 from dg = dY W2T^T (exact, never stored) and the saved interleaved h13: dh1 = dg sg a3 (1 + a1 (1 - sg)), dh3 = dg sg a1 with
    sg = sigmoid(a1), in the interleaved layout, within the bound of the module docstring (mag = |dg sg a3| (1 + |a1|) and |dh3|)."""
    route, M, H, Kd, ring_min = case
    threshold(monkeypatch, ring_min)
    dtype = F32 if route == "F32" else BF
    dy, w2t, dg, g = operands(M, H, Kd, dtype, seed=M + H + Kd + 1, w_scale=act_scale(Kd))
    h13f = torch.randint(-24, 25, (M, 2 * H), generator=g).float() / 8
    h13f[:, 3] += (torch.arange(M) % 5).float() / 4
    h13 = h13f.to(dtype).cuda()
    assert torch.equal(h13.float().cpu(), h13f)
    reaches(K, route, M, H, Kd, dtype, mode=2)
    dh13 = K.gemm_nt_dswiglu(dy, w2t, h13)
    if wants_pieces(route):
        for lo, hi in pieces(M):
            reaches(K, "NT_GLDS4", hi - lo, H, Kd, dtype, mode=2)
            assert torch.equal(dh13[lo:hi], K.gemm_nt_dswiglu(dy[lo:hi], w2t, h13[lo:hi])), f"rows {lo}..{hi} differ from the 128 x 128 kernel's"
    il = h13f.double().view(M, H // 4, 2, 4)
    a1, a3 = il[:, :, 0].reshape(M, H), il[:, :, 1].reshape(M, H)
    sg = torch.sigmoid(a1)
    d1, d3 = dg * sg * a3 * (1 + a1 * (1 - sg)), dg * sg * a1
    m1 = (dg * sg * a3).abs() * (1 + a1.abs())
    inter = lambda x, y: torch.stack([x.view(M, H // 4, 4), y.view(M, H // 4, 4)], dim=2).reshape(M, 2 * H)
    check_bound("swiglu_bwd", route, dh13, inter(d1, d3), inter(m1, d3.abs()), dtype)


@pytest.mark.parametrize("case", cases.NT_ROPE_CASES, ids=cid)
def test_rope(K, monkeypatch, case):
    """q|k|v projection (+ bias) with the first rot_cols columns rotated by table[sample][pos_off + token][(n % D) / 2] = (cos, sin), the
    first q_cols of them by the pre-scaled copy of the table.  per_sample: a 4-d table with angles drawn per sample (reading another
    sample's rows, or the wrong row after the wrap at a sample boundary, is a gross error); else one 3-d table for all samples.
    Rotated columns within the bound of the module docstring (mag = |re cos| + |im sin|), the others bit-equal to the exact product."""
    route, B, T, N, Kd, D, rot, off, qc, with_bias, per_sample, ring_min = case
    threshold(monkeypatch, ring_min)
    dtype = F32 if route == "F32" else BF
    M = B * T
    assert qc % D == 0 and rot % D == 0
    ad, wd, acc, g = operands(M, N, Kd, dtype, seed=M + N + Kd + D, w_scale=act_scale(Kd))
    bias = torch.randint(-4, 5, (N,), generator=g).float() / 4 if with_bias else None
    Tc = off + T + 2
    ang = torch.rand(*((B,) if per_sample else ()), Tc, D // 2, generator=g) * 6.2831
    tab32 = torch.stack([ang.cos(), ang.sin()], -1)
    both = torch.stack([tab32, tab32 * 0.1803]).contiguous().cuda()          # the pre-scaled copy lives in the same allocation
    tab, qtab = both[0], both[1]
    sl = (lambda t, b0, b1: t[b0:b1]) if per_sample else (lambda t, b0, b1: t)
    run = lambda b0, b1: K.gemm_nt_rope(ad[b0 * T:b1 * T], wd, None if bias is None else bias.to(dtype).cuda(), sl(tab, b0, b1), T, off, D, rot,
                                        q_cols=qc, q_table=sl(qtab, b0, b1) if qc else None)
    reaches(K, route, M, N, Kd, dtype, has_rope=True)
    out = run(0, B)
    if wants_pieces(route):
        for b0, b1 in ((0, B // 2), (B // 2, B)):
            reaches(K, "NT_GLDS4", (b1 - b0) * T, N, Kd, dtype, has_rope=True)
            assert torch.equal(out[b0 * T:b1 * T], run(b0, b1)), f"samples {b0}..{b1} differ from the 128 x 128 kernel's"
    y = acc + (bias.double() if bias is not None else 0.0)
    nh, nq = rot // D, qc // D
    t64 = both.cpu().double()[..., off:off + T, :, :]                          # [2, (B,) T, D / 2, 2]
    t64 = t64[:, :, :, None] if per_sample else t64[:, None, :, None]          # [2, B or 1, T, 1, D / 2, 2]
    cs = torch.cat([t64[i].expand(B, T, n, D // 2, 2) for i, n in ((1, nq), (0, nh - nq)) if n], 2)      # per head: the queries' pre-scaled pairs first
    yr = y[:, :rot].reshape(B, T, nh, D // 2, 2)
    re, im, c, s = yr[..., 0], yr[..., 1], cs[..., 0], cs[..., 1]
    ref = torch.stack([re * c - im * s, re * s + im * c], -1).reshape(M, rot)
    mag = torch.stack([(re * c).abs() + (im * s).abs(), (re * s).abs() + (im * c).abs()], -1).reshape(M, rot)
    check_bound("rope", route, out[:, :rot], ref, mag, dtype)
    assert torch.equal(out[:, rot:].float().cpu(), rounded(y[:, rot:], dtype))


# ----------------------------------------------------------------------------------------------- TN
@pytest.mark.parametrize("case", cases.TN_CASES, ids=cid)
def test_gemm_tn_exact(K, case):
    """C (fp32) (+)= A^T B on integer operands, bit-equal to float64: one split (the kernel writes / accumulates into C itself), several
    (slabs summed in order by reduce_slabs4_kernel), splits that start past M (all-zero slabs) and a last split of 3 rows, N1 / N2 that
    are no multiples of the tile; out= views with ldc > N2, with ldc % 4 != 0 and with a pointer that is 4- but not 16-byte aligned (both
    take the scalar reduce_slabs_kernel when there is more than one split), each with accumulate and untouched neighbouring columns."""
    kernel, dt, M, N1, N2, nsplit, rps = case
    dtype = BF if dt == "bf16" else F32
    assert K.gemm_tn_route(M, N1, N2, dtype) == (kernel, nsplit, rps)
    g = torch.Generator().manual_seed(M + N1)
    a = torch.randint(-2, 3, (M, N1 + 8), generator=g).float()
    b = torch.randint(-2, 3, (M, N2), generator=g).float()
    a[:, 3] += (torch.arange(M) % 5).float()
    b[:, 1] += (torch.arange(M) % 3).float()
    ad, bd = a.to(dtype).cuda()[:, :N1], b.to(dtype).cuda()               # A with row stride N1 + 8
    ref = a[:, :N1].double().t() @ b.double()
    assert float(ref.abs().max()) < 2 ** 24
    ref = ref.float()
    assert torch.equal(K.gemm_tn(ad, bd).cpu(), ref)
    acc = torch.zeros(N1, N2, device="cuda")
    acc.fill_(3.0)
    K.gemm_tn(ad, bd, out=acc, accumulate=True)
    assert torch.equal(acc.cpu(), ref + 3)
    # (columns of the buffer, first column of the view): ldc > N2 aligned; ldc % 4 != 0; pointer 4 bytes past a 16-byte boundary
    views = [(N2 + 16, 8)] if kernel else [(N2 + 16, 8), (N2 + 6, 4), (N2 + 8, 1)]
    for cols, c0 in views:
        for accumulate in (False, True):
            buf = torch.zeros(N1, cols, device="cuda")
            buf.fill_(3.0)
            view = buf[:, c0:c0 + N2]
            assert (view.stride(0) % 4 == 0 and view.data_ptr() % 16 == 0) == ((cols, c0) == (N2 + 16, 8))
            K.gemm_tn(ad, bd, out=view, accumulate=accumulate)
            got = buf.cpu()
            assert torch.equal(got[:, c0:c0 + N2], ref + 3 if accumulate else ref), (cols, c0, accumulate)
            assert bool((got[:, :c0] == 3).all()) and bool((got[:, c0 + N2:] == 3).all()), (cols, c0, accumulate)
