"""The four token-on-the-lane kernels of csrc/mlp_fused.hip — mlp_up_fused_kernel and qkv_rope_fused_kernel (what fk_gemm_nt_swiglu /
fk_gemm_nt_rope run from 45 825 rows on at d = 384), mlp_bwd_fused_kernel and mlp_bwd_fused_asm_kernel (fk_mlp_bwd_fused) — against a
float64 reference on the CPU, every element.

Before it launches, every test asks the host-side query (kernels.gemm_nt_swiglu_route / gemm_nt_rope_route / mlp_bwd_fused_route) with
the pointers and leading dimensions it is about to pass and compares the answer with the route its case names: a moved threshold, or
a buffer the predicate rejects, fails the test instead of silently sending it through the tiled kernels (tests/test_lane_routes_cpu.py
pins the same table without a GPU; the shapes live in tests/cases.py, the references in tests/lane_ref.py).

Inputs are those of tests/test_gemm_routes_gpu.py (`operands`: integers in [-2, 2], an asymmetric ramp in one column of each operand,
weights scaled by act_scale's power of two, A with row stride K + 8; every product exact in fp32, asserted); for the backward also h13
in multiples of 1/8 with a ramp column and a w13t with a ramp along 2H and one along d.  The CPU file shows on the reference alone that
a dropped k block, a neighbouring chunk's weights, swapped h1 / h3, a neighbouring token's row, a neighbouring position's or sample's
rotation, the unscaled table on a query head and a confused leading dimension each move an element past the bound.

The bound is check_bound of tests/test_gemm_routes_gpu.py, imported:   |got - ref| <= 2^-8 |ref| + 2e-5 + 2e-5 mag
  * h13 and the unrotated q|k|v columns (every column at rot_cols = 0) must be BIT-EQUAL to the float64 product rounded once;
  * g (mag = |g|), rotated columns (mag = |re cos| + |im sin|) and dh13 (mag = |dg sg a3| (1 + |a1|), |dh3|) use that file's magnitudes;
  * dx is held to float64(dh13 as the kernel stored it) @ float64(w13t) — dh13 meets float64 on its own in the same test — with
    mag = |dh13| @ |w13t| and the relative factor max(2e-5, 2H * 2^-24), the worst case of an fp32 sum of 2H terms (2e-5 up to H = 160).
Outputs live in sentinel-filled allocations of their own, 16 bytes in: everything around the [M, N] block must still hold the sentinel.

Each check prints "FRAC <what> NT_LANE <largest error / bound>".  Largest fractions on the MI355X (CPU model of the documented
arithmetic in brackets, tests/test_lane_routes_cpu.py):
    up-projection g        0.9833 (0.9833)   padded 0.9833          saturated 0.9833 (0.9833), its saturated units alone 0.9758 (0.9758)
    rotated q|k|v columns  0.9904 (0.9904)   padded 0.9894
    dh13, both kernels     0.9833 (0.9833)   padded 0.9809          saturated 0.9762 hipcc / 0.9713 stream (0.9762), units 0.9261 (0.9261)
    dx, both kernels       0.9855 (0.9855)   padded 0.9718          saturated 0.9831 hipcc / 0.9805 stream (0.9831)
The fractions are those of the bf16 rounding of the stored value (2^-8 |ref| is half an ulp just above a power of two, so rounding alone
reaches 0.98 .. 0.99 of it somewhere in 10^6 .. 10^7 elements); the kernels' fp32 arithmetic moves the fourth digit at most.
"""
import functools

import pytest
import torch

from tests import cases, lane_ref as LR
from tests.test_gemm_routes_gpu import act_scale, check_bound, operands, rounded

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = -7.0
d = cases.LANE_D
TAIL = 4096                                                 # sentinel elements behind the last row ("rows past M")


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    assert act_scale(d) == LR.W_SCALE
    return kernels


def cid(c):
    return "-".join(str(x) for x in c)


class Framed:
    """an [R, C] bf16 block with leading dimension C + pad that starts `lead` elements (a multiple of 8: 16-byte aligned, but not the
    allocation's base) into a sentinel-filled allocation with TAIL more elements behind the last row; src: its contents (a CPU tensor)"""

    def __init__(self, R, C, pad=0, lead=8, src=None):
        assert lead % 8 == 0 and pad % 8 == 0
        self.shape, self.ld, self.lead = (R, C), C + pad, lead
        self.flat = torch.full((lead + R * self.ld + TAIL,), SENTINEL, dtype=BF, device="cuda")
        self.view = self._block(self.flat)
        if src is not None:
            assert tuple(src.shape) == (R, C) and torch.equal(src.to(BF).float(), src.float())
            self.view.copy_(src.to(BF))
        assert self.view.data_ptr() % 16 == 0 and self.view.data_ptr() != self.flat.data_ptr()

    def _block(self, flat):
        return flat.as_strided(self.shape, (self.ld, 1), self.lead)

    def untouched(self):
        """padding columns, the elements in front and every row past the block still hold the sentinel"""
        c = self.flat.clone()
        self._block(c).fill_(SENTINEL)
        return bool((c == SENTINEL).all())

    def cpu(self):
        return self.view.float().cpu()


def aligned(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


def run_up(K, a, w13, M, H, pads=(0, 0), leads=(8, 8)):
    """fk_gemm_nt_swiglu on raw pointers into framed outputs, after the route query has said NT_LANE for exactly this call"""
    from frankenstein_amd._lib import call
    h13, g = Framed(M, 2 * H, pads[0], leads[0]), Framed(M, H, pads[1], leads[1])
    route = K.gemm_nt_swiglu_route(M, H, d, a.stride(0), w13.stride(0), h13.ld, g.ld, aligned(a, w13, h13.view, g.view), BF)
    assert K.NT_ROUTE_NAMES[route] == "NT_LANE", K.NT_ROUTE_NAMES[route]
    call("fk_gemm_nt_swiglu", a.data_ptr(), a.stride(0), w13.data_ptr(), w13.stride(0), h13.view.data_ptr(), h13.ld, g.view.data_ptr(), g.ld,
         M, H, d, K.fk_dtype(BF), K._stream())
    assert h13.untouched() and g.untouched(), "a store outside the [M, 2H] / [M, H] blocks"
    return h13, g


def run_qkv(K, a, w, both, B, T, N, rot, qc, off, per_sample, pad=0, lead=8):
    from frankenstein_amd._lib import call
    M = B * T
    out = Framed(M, N, pad, lead)
    tab, qtab = both[0], both[1]
    assert both.is_contiguous() and both.dtype == torch.float32 and tab.shape[-3] == off + T
    tbs = tab.stride(0) if per_sample else 0
    q_off = (qtab.data_ptr() - tab.data_ptr()) // 4 if qc else 0
    route = K.gemm_nt_rope_route(M, N, d, T, LR.HEAD, rot, qc, off, False, a.stride(0), w.stride(0), out.ld, aligned(a, w, out.view, tab), BF)
    assert K.NT_ROUTE_NAMES[route] == "NT_LANE", K.NT_ROUTE_NAMES[route]
    call("fk_gemm_nt_rope", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.view.data_ptr(), out.ld, M, N, d, None,
         tab.data_ptr(), tbs, T, off, LR.HEAD, rot, qc, q_off, K.fk_dtype(BF), K._stream())
    assert out.untouched(), "a store outside the [M, N] block"
    return out


def run_bwd(K, kernel, dy, w2t, h13, w13t, M, H, pads=(0, 0), leads=(8, 8)):
    from frankenstein_amd._lib import call
    dh, dx = Framed(M, 2 * H, pads[0], leads[0]), Framed(M, d, pads[1], leads[1])
    assert aligned(dy, w2t, h13, w13t, dh.view, dx.view)
    route = K.MLP_BWD_ROUTE_NAMES[K.mlp_bwd_fused_route(M, dh.ld)]
    assert route == kernel, f"{M} rows with lddh {dh.ld} reach {route}, not {kernel}"
    call("fk_mlp_bwd_fused", dy.data_ptr(), dy.stride(0), w2t.data_ptr(), w2t.stride(0), h13.data_ptr(), h13.stride(0), w13t.data_ptr(),
         w13t.stride(0), dh.view.data_ptr(), dh.ld, dx.view.data_ptr(), dx.ld, M, H, d, K.fk_dtype(BF), K._stream())
    assert dh.untouched() and dx.untouched(), "a store outside the [M, 2H] / [M, d] blocks"
    return dh, dx


def check_up(tag, h13, g, acc):
    assert torch.equal(h13.cpu(), rounded(acc, BF)), "h13 is not the exact product rounded once"
    ref = LR.up_ref(acc)
    check_bound(tag, "NT_LANE", g.view, ref, ref.abs(), BF)


def check_qkv(tag, out, acc, both, B, T, N, rot, qc, off, per_sample):
    got = out.cpu()
    if rot:
        c, s = LR.rope_pairs(both.cpu(), B, T, N, rot, qc, off, per_sample)
        ref, mag = LR.qkv_ref(acc, c, s, B, T, rot)
        check_bound(tag, "NT_LANE", got[:, :rot], ref[:, :rot], mag[:, :rot], BF)
    assert torch.equal(got[:, rot:], rounded(acc[:, rot:], BF)), "an unrotated column is not the exact product rounded once"


def check_bwd(tag, kernel, dh, dx, dg, h13, w13t):
    ref, mag = LR.bwd_ref(dg, h13)
    check_bound(f"{tag}[{kernel}]", "NT_LANE", dh.view, ref, mag, BF)
    xref, xmag, relf = LR.dx_ref(dh.cpu(), w13t)
    check_bound(f"{'dx' if tag == 'swiglu_bwd' else tag + '_dx'}[{kernel}]", "NT_LANE", dx.view, xref, xmag * (relf / 2e-5), BF)


def test_the_cpu_file_checks_the_inputs_these_tests_run(K):
    """lane_ref.operands_cpu (whose values tests/test_lane_routes_cpu.py holds against the mutations) is test_gemm_routes_gpu.operands"""
    for M, N, seed in ((300, 64, LR.up_seed(300, 32)), (129, 192, LR.qkv_seed(129, 192))):
        ad, wd, ref, g = operands(M, N, d, BF, seed=seed, w_scale=act_scale(d))
        a, w, acc, g2 = LR.operands_cpu(M, N, d, seed, LR.W_SCALE)
        assert ad.stride(0) == d + 8 and torch.equal(ad.float().cpu(), a) and torch.equal(wd.float().cpu(), w) and torch.equal(ref, acc)
        assert torch.equal(torch.rand(5, generator=g), torch.rand(5, generator=g2))


# ----------------------------------------------------------------------------------------------- float64, every element
@pytest.mark.parametrize("case", cases.LANE_UP_CASES, ids=cid)
def test_up_projection_float64(K, case):
    """h13 = A W13^T (interleaved: per 4 hidden units 4 columns of h1, then 4 of h3) bit-equal to the exact product rounded once,
    g = silu(h1) h3 from the unrounded accumulator within the bound: 1, 2, 3 and 5 chunks; one row in the last workgroup, whole
    workgroups, a row count that cuts an 8-row h13 store group and a 16-row g group; two rounds of workgroups"""
    _, M, H = case
    ad, w13, acc, _ = operands(M, 2 * H, d, BF, seed=LR.up_seed(M, H), w_scale=act_scale(d))
    h13, g = run_up(K, ad, w13, M, H)
    check_up("swiglu_fwd", h13, g, acc)


@pytest.mark.parametrize("case", cases.LANE_QKV_CASES, ids=cid)
def test_qkv_rope_float64(K, case):
    """q|k|v projection with the first rot_cols columns rotated by table[sample][pos_off + token] (the first q_cols by the pre-scaled
    copy): 1, 3 and 6 heads; nothing, everything, everything pre-scaled, and q | k | v thirds; one token per sample, one sample, T = 975
    (workgroups straddle samples) and T = 3 (85 samples per workgroup); tables of exactly pos_off + T rows, shared and per sample"""
    _, B, T, N, rot, qc, off, per_sample = case
    M = B * T
    ad, wd, acc, g = operands(M, N, d, BF, seed=LR.qkv_seed(M, N), w_scale=act_scale(d))
    both = LR.rope_tables(g, B, T, off, per_sample).cuda()
    out = run_qkv(K, ad, wd, both, B, T, N, rot, qc, off, per_sample)
    check_qkv("rope", out, acc, both, B, T, N, rot, qc, off, per_sample)


@functools.lru_cache(maxsize=2)
def bwd_inputs(H):
    return LR.bwd_operands(H, cases.LANE_BWD_ROWS)


def bwd_case(K, kernel, M, H):
    dy, w2t, dg, h13, w13t = (t[:M] if t.shape[0] == cases.LANE_BWD_ROWS else t for t in bwd_inputs(H))
    up = lambda t, pad: Framed(t.shape[0], t.shape[1], pad, src=t).view
    dh, dx = run_bwd(K, kernel, up(dy, 8), up(w2t, 0), up(h13, 0), up(w13t, 0), M, H)
    return dh, dx, dg, h13, w13t


@pytest.mark.parametrize("case", cases.LANE_BWD_CASES, ids=cid)
def test_mlp_backward_chain_float64(K, case):
    """dh13 = SwiGLU'(h13) (dy W2T^T) and dx = dh13 W13T^T in one launch, on the kernel the case names: 1 .. 5 chunks (4: the first count at
    which the generated stream's chunk clamp is both idle and active in one run); 1, 7, 33 and 127 rows (every load of the workgroup
    clamped), 129, 393 and 1000 (a partial last wave, a cut 8-row store group), whole tiles on the generated stream.  The 255-row case
    (hipcc kernel) must also give the bits of the first 255 rows of the 256-row case (generated stream) on the same operands."""
    kernel, M, H = case
    dh, dx, dg, h13, w13t = bwd_case(K, kernel, M, H)
    check_bwd("swiglu_bwd", kernel, dh, dx, dg, h13, w13t)
    if case == cases.LANE_BWD_PAIR[1]:
        k2, M2, _ = cases.LANE_BWD_PAIR[0]
        assert M2 == M + 1 and k2 != kernel
        dh2, dx2, *_ = bwd_case(K, k2, M2, H)
        assert torch.equal(dh.view, dh2.view[:M]) and torch.equal(dx.view, dx2.view[:M]), "the two backward kernels differ on the same rows"


# ----------------------------------------------------------------------------------------------- padded leading dimensions
def test_padded_leading_dimensions_up_projection(K):
    """every operand and output in a wider sentinel-filled buffer with a pad of its own (no two leading dimensions equal) and a base that
    is 16-byte aligned but not its allocation's: the bits of the contiguous call, inside the float64 bound, the sentinels untouched"""
    M, H, (pa, pw, ph, pg) = cases.LANE_PAD_UP
    a, w, acc, _ = LR.operands_cpu(M, 2 * H, d, LR.up_seed(M, H), LR.W_SCALE)
    h13, g = run_up(K, Framed(M, d, pa, 8, a).view, Framed(2 * H, d, pw, 16, w).view, M, H, (ph, pg), (24, 32))
    assert len({d + pa, d + pw, h13.ld, g.ld}) == 4
    h13c, gc = run_up(K, a.to(BF).cuda(), w.to(BF).cuda(), M, H)
    assert torch.equal(h13.view, h13c.view) and torch.equal(g.view, gc.view), "padded and contiguous calls differ"
    check_up("swiglu_fwd_padded", h13, g, acc)


def test_padded_leading_dimensions_qkv_rope(K):
    B, T, N, rot, qc, off, per_sample, (pa, pw, po) = cases.LANE_PAD_QKV
    M = B * T
    a, w, acc, gen = LR.operands_cpu(M, N, d, LR.qkv_seed(M, N), LR.W_SCALE)
    both = LR.rope_tables(gen, B, T, off, per_sample).cuda()
    out = run_qkv(K, Framed(M, d, pa, 8, a).view, Framed(N, d, pw, 16, w).view, both, B, T, N, rot, qc, off, per_sample, po, 24)
    assert len({d + pa, d + pw, out.ld}) == 3
    outc = run_qkv(K, a.to(BF).cuda(), w.to(BF).cuda(), both, B, T, N, rot, qc, off, per_sample)
    assert torch.equal(out.view, outc.view), "padded and contiguous calls differ"
    check_qkv("rope_padded", out, acc, both, B, T, N, rot, qc, off, per_sample)


@pytest.mark.parametrize("case", cases.LANE_PAD_BWD, ids=lambda c: cid(c[:2]))
def test_padded_leading_dimensions_mlp_backward(K, case):
    M, H, (py, p2, ph, p13, pdh, pdx) = case
    kernel = "MLP_BWD_ASM" if M % 128 == 0 else "MLP_BWD_HIPCC"
    dy, w2t, dg, h13, w13t = (t[:M] if t.shape[0] == cases.LANE_BWD_ROWS else t for t in bwd_inputs(H))
    fr = lambda t, pad, lead: Framed(t.shape[0], t.shape[1], pad, lead, t).view
    dh, dx = run_bwd(K, kernel, fr(dy, py, 8), fr(w2t, p2, 16), fr(h13, ph, 24), fr(w13t, p13, 32), M, H, (pdh, pdx), (40, 48))
    assert len({d + py, d + p2, 2 * H + ph, 2 * H + p13, dh.ld, dx.ld}) == 6
    dhc, dxc = run_bwd(K, kernel, *(t.to(BF).cuda() for t in (dy, w2t, h13, w13t)), M, H)
    assert torch.equal(dh.view, dhc.view) and torch.equal(dx.view, dxc.view), "padded and contiguous calls differ"
    check_bwd("swiglu_bwd_padded", kernel, dh, dx, dg, h13, w13t)


# ----------------------------------------------------------------------------------------------- saturated gates
def test_saturated_gates_forward(K):
    """pre-activations of exactly +-{8, 16, 32, 64, 88, 96, 128} (and +-1) on both sides of __expf's overflow at 88.72, against h3 of
    mixed sign and size: activation column 9 is the constant 1 and the h1 weight rows of the chosen units hold the value in column 9
    alone, so the accumulator is that value exactly.  g finite and inside the bound, h13 bit-equal."""
    M, H = 45825, 32
    a, w, acc, pre = LR.saturated_up_operands(M, H, cases.LANE_SATURATED)
    h13, g = run_up(K, Framed(M, d, 8, 8, a).view, w.to(BF).cuda(), M, H)
    assert bool(torch.isfinite(g.view).all())
    check_up("saturated_fwd", h13, g, acc)
    sat = [u for u, v in enumerate(pre) if abs(v) > 1]
    ref = LR.up_ref(acc)[:, sat]
    check_bound("saturated_fwd_units", "NT_LANE", g.view[:, sat], ref, ref.abs(), BF)


@pytest.mark.parametrize("M", [128, 129])
def test_saturated_gates_backward(K, M):
    """the same pre-activations written into h13 directly, on both backward kernels: 1 + a1 (1 - sg) with sg = rcp(1 + exp(-a1))"""
    H = 32
    kernel = "MLP_BWD_ASM" if M % 128 == 0 else "MLP_BWD_HIPCC"
    dy, w2t, dg, h13, w13t, pre = LR.saturated_bwd_operands(H, M, cases.LANE_SATURATED)
    dh, dx = run_bwd(K, kernel, *(t.to(BF).cuda() for t in (dy, w2t, h13, w13t)), M, H)
    assert bool(torch.isfinite(dh.view).all()) and bool(torch.isfinite(dx.view).all())
    check_bwd("saturated_bwd", kernel, dh, dx, dg, h13, w13t)
    cols = [8 * (u // 4) + u % 4 + o for u, v in enumerate(pre) if abs(v) > 1 for o in (0, 4)]
    ref, mag = LR.bwd_ref(dg, h13)
    check_bound(f"saturated_bwd_units[{kernel}]", "NT_LANE", dh.view[:, cols], ref[:, cols], mag[:, cols], BF)
