"""The edges of the envelope the C ABI declares (include/franken_hip.h), on the MI355X: shapes the argument checks admit and no other test
runs.  References are the plain CPU formulation (oracle/ref_models.py, float64 where it is cheap) on the same bf16-rounded operands; the
tolerances are those the existing tests of the same quantity use (tests/test_kernels_gpu.py), not new ones.

    limit                                        checked in                                   inside (runs, must be right)                         outside (must be refused)
    -------------------------------------------  -------------------------------------------  ---------------------------------------------------  ------------------------------------------------
    attention head_dim 128: bf16 only            check_common, csrc/attention.hip             test_attention_d128_* / test_block_stack_d128_*      test_attention_d128_fp32_is_refused
    fk_attn_decode head_dim in {16,32,64,128}    fk_attn_decode, csrc/decode.hip              test_attn_decode_against_float64_softmax             (tests/test_kernels_gpu.py::test_errors_are_loud)
    fk_mlp_bwd_fused: M * ldh * 2 < 2^32 bytes   fk_mlp_bwd_fused, csrc/mlp_fused.hip         test_mlp_bwd_fused_offsets_past_2gib (2.25 GiB)      test_mlp_bwd_fused_refuses_offsets_past_4gib
      its mirror: rows * 2H * 2 < 2^32           MlpBranch.backward, engine.py                test_mlp_module_routing_...[393216]                  test_mlp_module_routing_...[700032] (two GEMMs)
    bf16 D = 64 attention: row strides < 2^24,   check_common, csrc/attention.hip             test_attention_d64_large_row_stride (3.9 GiB from    test_attention_d64_stride_limits_are_refused
      head slab rs * N < 2^31 elements                                                          the base), .._largest_24_bit_stride (2^24 - 8)
    token-on-the-lane fast paths: N, H > 0,      fk_qkv_rope_fused_ok / fk_mlp_up_fused_ok,   tests/test_kernels_gpu.py (bit-for-bit tests)        test_fast_paths_leave_bad_arguments_to_launch_nt
      leading dimensions cover their rows          csrc/mlp_fused.hip; launch_nt, csrc/gemm.hip

Every large buffer is filled with NaN before the operands are written into it, and after the call the NaNs outside the written region are
counted on the device: a load from a wrong address poisons the result, a store to a wrong address inside the buffer changes the count.
Stores outside it are caught by the guard bands of tests/poison.py where the buffer is small enough to be tracked."""
import math

import pytest
import torch

from oracle import ref_models as R
from tests import test_kernels_gpu as TK
from tests.test_kernels_gpu import close, dev, mask_tensor, q, ref_attn, rnd

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


@pytest.fixture(autouse=True)
def _release_big_blocks():
    """the multi-GiB buffers of one test go back to the driver before the next one asks for blocks of another size"""
    yield
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def nan_count(t):
    return int(torch.isnan(t).sum())


# =============================================================================================== A. head_dim = 128, bf16
ATTN_D128_CASES = [
    # B, H, Nq, Nk, D, kind, c        (tests/test_kernels_gpu.py::ATTN_CASES at D = 128)
    (2, 3, 128, 128, 128, 0, 0),
    (1, 2, 200, 200, 128, 2, 8),
    (2, 2, 57, 57, 128, 1, 0),
    (1, 1, 320, 320, 128, 1, 0),
    (1, 4, 32, 300, 128, 0, 0),
    (2, 4, 40, 128, 128, 2, 16),
    (1, 2, 8, 8, 128, 0, 0),
    (1, 2, 512, 512, 128, 2, 256),
]


@pytest.mark.parametrize("case", ATTN_D128_CASES)
def test_attention_d128_fwd_bwd(K, case):
    """forward, LSE, dQ, dK, dV against the oracle: the body (q in its own buffer, k|v packed side by side) and the tolerances of
    test_attention_fwd_bwd (forward 2e-2, LSE 3e-2, gradients 4e-2)."""
    TK.test_attention_fwd_bwd(K, BF16, case)


def test_attention_d128_dense_boolean_mask(K):
    """one mask per sample and per head, with the wholly masked leading tiles, the key nobody sees and its exact-zero dK / dV row"""
    TK.test_attention_dense_boolean_mask(K, BF16, (2, 3, 130, 200, 128, True, True))


def test_attention_d128_dropout_same_draw(K):
    TK.test_attention_dropout_matches_the_oracle_with_the_same_draw(K, BF16, (2, 2, 200, 200, 128, 1, 0, 0.1))


def _fwd_bwd_against(K, qv, kv, vv, do, mask, oref_fn):
    """bf16 forward + backward of [B, N, H, D] operands under `mask`; oref_fn(qr, kr, vr) -> oracle output.  The tolerances of
    test_attention_fwd_bwd."""
    qd, kd, vd = dev(qv, BF16), dev(kv, BF16), dev(vv, BF16)
    o, lse = K.attn_fwd(qd, kd, vd, mask)
    qr, kr, vr = (q(t_, BF16).requires_grad_(True) for t_ in (qv, kv, vv))
    oref = oref_fn(qr, kr, vr)
    close(o, oref, BF16, atol16=2e-2)
    (oref * q(do, BF16)).sum().backward()
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    K.attn_bwd(qd, kd, vd, o, dev(do, BF16), lse, dq, dk, dv, mask)
    close(dq, qr.grad, BF16, atol16=4e-2)
    close(dk, kr.grad, BF16, atol16=4e-2)
    close(dv, vr.grad, BF16, atol16=4e-2)
    return o, lse


def test_attention_d128_prefix_mask_from_token_ids(K):
    B, H, N, n, D, Cb = 2, 2, 512, 200, 128, 16
    ids = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(10 + i))[:n].sort()[0] for i in range(B)])
    m = K.Mask.from_token_ids(dev(ids), dev(ids), Cb)
    dense = (ids[:, None, :] // Cb) <= (ids[:, :, None] // Cb)
    qv, kv, vv, do = (rnd(B, n, H, D, seed=s) for s in (1, 2, 3, 4))
    _fwd_bwd_against(K, qv, kv, vv, do, m, lambda a, b, c: ref_attn(a, b, c, dense[:, None]))


def test_attention_d128_key_padding(K):
    """Mask.from_padding: padded tail, holes, and fully masked query rows (0 in the oracle's torch >= 2.1 form)"""
    B, H, N, D = 2, 2, 260, 128
    valid = torch.ones(B, N, dtype=torch.bool)
    valid[0, 200:] = False
    valid[1, 37:41] = False
    pad = (valid[:, None, :, None] & valid[:, None, None, :])
    m = K.Mask.from_padding(dev(valid), dev(valid))
    qv, kv, vv, do = (rnd(B, N, H, D, seed=s) for s in (1, 2, 3, 4))
    _fwd_bwd_against(K, qv, kv, vv, do, m, lambda a, b, c: R.sdpa_zero_fully_masked(
        a.transpose(1, 2), b.transpose(1, 2), c.transpose(1, 2), pad.expand(B, 1, N, N)).transpose(1, 2))


def test_attention_d128_mask_offsets_and_spike(K):
    """Mask.sliced (t_q < t_k) and a late key that makes the running maximum jump"""
    B, H, Nq, Nk, D = 1, 2, 40, 200, 128
    qv, kv, vv, do = rnd(B, Nq, H, D, seed=1), rnd(B, Nk, H, D, seed=2), rnd(B, Nk, H, D, seed=3), rnd(B, Nq, H, D, seed=4)
    kv[0, 150, 0] = 6.0 * qv[0, 7, 0]
    m = K.Mask(2, 8).sliced(256, 256, Nq, Nk)
    mt = mask_tensor(2, 8, 256, 256)[-Nq:, -Nk:]
    _fwd_bwd_against(K, qv, kv, vv, do, m, lambda a, b, c: ref_attn(a, b, c, mt))


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_rope_and_projection_epilogue_d128(K, dtype):
    """fk_rope and the fk_gemm_nt_rope epilogue at head_dim 128 against R.apply_rope (the bodies and tolerances of test_rope and
    test_fused_rope_projection_and_backward)"""
    B, T, H, D, d = 2, 50, 2, 128, 64
    ang = R.rope_angles(D, 64, 10000.0)
    table = torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous()
    x = rnd(B, T, 3 * H * D, seed=1)
    xd = dev(x, dtype)
    K.rope_(xd, 2 * H, D, dev(table), pos_off=64 - T)
    want = q(x, dtype).clone()
    want[..., : 2 * H * D] = R.apply_rope(want[..., : 2 * H * D].reshape(B, T, 2 * H, D), ang).reshape(B, T, -1)
    close(xd, want, dtype, atol32=1e-6, atol16=2e-2)
    if dtype == torch.float32:
        K.rope_(xd, 2 * H, D, dev(table), pos_off=64 - T, conj=True)
        close(xd, x, dtype, atol32=1e-5)
    xin, w, bias = rnd(B * T, d, seed=2), rnd(3 * H * D, d, seed=3, scale=0.2), rnd(3 * H * D, seed=4, scale=0.1)
    got = K.gemm_nt_rope(dev(xin, dtype), dev(w, dtype), dev(bias, dtype), dev(table), T, 64 - T, D, 2 * H * D)
    ref = (q(xin, dtype) @ q(w, dtype).t() + q(bias, dtype)).view(B, T, 3 * H * D)
    ref[..., : 2 * H * D] = R.apply_rope(ref[..., : 2 * H * D].reshape(B, T, 2 * H, D), ang).reshape(B, T, -1)
    close(got.view(B, T, -1), ref, dtype, atol32=2e-5, atol16=3e-2)


def test_attention_d128_fused_rope_backward(K):
    """attn_bwd(..., rope_table=) == attn_bwd followed by rope_(conj=True), as test_fused_rope_projection_and_backward holds it at D = 16"""
    B, T, H, D = 2, 40, 2, 128
    ang = R.rope_angles(D, 64, 10000.0)
    table = dev(torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous())
    qkv = dev(rnd(B, T, 3 * H * D, seed=4), BF16)
    qv, kv, vv = (qkv[..., i * H * D:(i + 1) * H * D].unflatten(-1, (H, D)) for i in range(3))
    o, lse = K.attn_fwd(qv, kv, vv, K.Mask(1))
    do = dev(rnd(B, T, H, D, seed=5), BF16)
    d1, d2 = torch.empty_like(qkv), torch.empty_like(qkv)
    views = lambda t: [t[..., i * H * D:(i + 1) * H * D].unflatten(-1, (H, D)) for i in range(3)]
    K.attn_bwd(qv, kv, vv, o, do, lse, *views(d1), K.Mask(1))
    K.rope_(d1, 2 * H, D, table, 64 - T, conj=True)
    K.attn_bwd(qv, kv, vv, o, do, lse, *views(d2), K.Mask(1), rope_table=table, rope_off=64 - T)
    close(d2, d1.float().cpu(), BF16, atol16=3e-2)


def test_block_stack_d128_matches_oracle_in_bf16():
    """Two brainformer Blocks with head_dim 128 (dim 256, 2 heads; RoPE, block-causal mask, ragged token count) in bf16 mode against the fp32
    oracle: output within test_bf16_drift_small's bound (0.15), the input gradient and every parameter gradient finite and, as the other
    bf16 block tests ask (test_block_without_rope_takes_the_prescaled_kernels_in_bf16), with cosine >= 0.99 / 0.995 to the oracle's."""
    import frankenstein_amd as fa
    from frankenstein_amd import synth
    from frankenstein_amd.models import brainformer as bf
    cfg = bf.MAEConfig(window_size=8, n_electrodes=8, patch_size=4, dim=256, n_layers=2, head_dim=128, hidden_dim=512, n_heads=2, n_kv_heads=2)
    T, Tc = 200, 256
    blocks = torch.nn.ModuleList([bf.Block(cfg) for _ in range(2)])
    st = synth.make_state({k: tuple(v.shape) for k, v in blocks.state_dict().items()})
    blocks.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    blocks.cuda()
    sd = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in st.items()}
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(2, T, 256, generator=g), torch.randn(2, T, 256, generator=g)
    ang = R.rope_angles(128, Tc, 10000.0)
    xr = x.clone().requires_grad_(True)
    want = xr
    for i in range(2):
        want = R.block(sd, f"{i}.", want, cfg, R.block_causal_mask(Tc, 8), ang)
    (want * dy).sum().backward()
    mask = bf.build_advanced_causal_mask(Tc, 8)
    rope = bf.build_complex_rope_cache(128, Tc, 10000.0).cuda()
    fa.set_compute_dtype("bf16")
    try:
        xd = x.cuda().requires_grad_(True)
        out = xd
        for blk in blocks:
            out = blk(out, attn_mask=mask, rope=rope)
        (out.float() * dy.cuda()).sum().backward()
    finally:
        fa.set_compute_dtype("bf16")
    err = float((out.float().cpu() - want).abs().max())
    print(f"block stack D=128: max |out - oracle| = {err:.4f}")
    assert err < 0.15
    cos = lambda a, b: float((a.flatten().double() @ b.flatten().double()) / (a.norm().double() * b.norm().double() + 1e-30))
    dx = xd.grad.float().cpu()
    assert bool(torch.isfinite(dx).all()) and cos(dx, xr.grad) > 0.995, cos(dx, xr.grad)
    for k, p in blocks.named_parameters():
        gk = p.grad.float().cpu()
        assert bool(torch.isfinite(gk).all()) and cos(gk, sd[k].grad) > 0.99, (k, cos(gk, sd[k].grad))


def test_attention_d128_fp32_is_refused(K):
    from frankenstein_amd._lib import FrankenHipError
    z = torch.zeros(1, 8, 1, 128, device="cuda")
    with pytest.raises(FrankenHipError, match="head_dim"):
        K.attn_fwd(z, z, z)
    with pytest.raises(FrankenHipError, match="head_dim"):
        K.attn_bwd(z, z, z, z, z, torch.zeros(1, 1, 8, device="cuda"), torch.empty_like(z), torch.empty_like(z), torch.empty_like(z))


# =============================================================================================== B. offsets past 2 GiB
MF_D, MF_H = 384, 1536
SLACK = 128                                             # NaN rows in front of and behind every big operand / result


def _mlp_chain_f64(dy, w2t, h13):
    """float64 dh13 [m, 2H] (interleaved: per 4 units 4 x d h1, then 4 x d h3) of the SwiGLU backward, from CPU tensors"""
    m, H = dy.shape[0], w2t.shape[0]
    dg = dy.double() @ w2t.double().t()
    hh = h13.double().view(m, H // 4, 2, 4)
    a1, a3 = hh[:, :, 0].reshape(m, H), hh[:, :, 1].reshape(m, H)
    sg = torch.sigmoid(a1)
    d1, d3 = dg * sg * a3 * (1 + a1 * (1 - sg)), dg * sg * a1
    return torch.stack([d1.view(m, H // 4, 4), d3.view(m, H // 4, 4)], dim=2).reshape(m, 2 * H)


def _check_mlp_rows(lo, hi, dy, w2t, h13, w13t, dh, dx):
    """rows lo:hi of the kernel's dh13 / dx against the float64 chain on the CPU; atol / rtol of
    test_mlp_backward_fused_equals_the_two_gemm_kernels_bit_for_bit (dx from the dh13 the kernel rounded to bf16, as there)"""
    c = lambda t: t.float().cpu()
    want = _mlp_chain_f64(c(dy[lo:hi]), c(w2t), c(h13[lo:hi]))
    got = c(dh[lo:hi])
    print(f"rows {lo}:{hi}  max |dh13 - f64| = {float((got.double() - want).abs().max()):.4g}")
    torch.testing.assert_close(got, want.float(), atol=3e-2, rtol=2e-2)
    want_dx = (got.double() @ c(w13t).double().t()).float()
    print(f"rows {lo}:{hi}  max |dx - f64| = {float((c(dx[lo:hi]) - want_dx).abs().max()):.4g}")
    torch.testing.assert_close(c(dx[lo:hi]), want_dx, atol=3e-2, rtol=2e-2)


@pytest.mark.parametrize("M", [393216, 393216 + 37])
def test_mlp_bwd_fused_offsets_past_2gib(K, M):
    """fk_mlp_bwd_fused with M * ldh * 2 = 2.25 GiB: the 32-bit byte offsets from the h13 / dh13 base (hoff[], ofs[6..13]) pass 2^31 at row
    349 525.  393 216 rows (whole 128-token tiles) take the generated-stream kernel, 393 253 the plain one, whose clamped tail rows sit at
    the highest offset of all.  dh13 and dx are the bits of fk_gemm_nt_dswiglu + fk_gemm_nt over the whole tensor, three blocks of 4096
    rows (first, the one where the offset crosses 2^31, last) meet the float64 chain, and no NaN of the surrounding rows moves."""
    from frankenstein_amd._lib import call
    assert 2 ** 31 < M * 2 * MF_H * 2 < 2 ** 32
    gen = torch.Generator(device="cuda").manual_seed(M)
    w2t = (torch.randn(MF_H, MF_D, device="cuda", generator=gen) / math.sqrt(MF_D)).bfloat16()
    w13t = (torch.randn(MF_D, 2 * MF_H, device="cuda", generator=gen) / math.sqrt(MF_H)).bfloat16()
    rows = M + 2 * SLACK
    bufs = {}
    for name, cols in (("dy", MF_D), ("h13", 2 * MF_H), ("dh", 2 * MF_H), ("dx", MF_D)):
        bufs[name] = torch.full((rows, cols), float("nan"), dtype=BF16, device="cuda")
    dy, h13, dh, dx = (bufs[n][SLACK:SLACK + M] for n in ("dy", "h13", "dh", "dx"))
    dy.normal_(0.0, 0.5, generator=gen)
    h13.normal_(0.0, 1.0, generator=gen)
    call("fk_mlp_bwd_fused", dy.data_ptr(), MF_D, w2t.data_ptr(), MF_D, h13.data_ptr(), 2 * MF_H, w13t.data_ptr(), 2 * MF_H,
         dh.data_ptr(), 2 * MF_H, dx.data_ptr(), MF_D, M, MF_H, MF_D, K.fk_dtype(dy), K._stream())
    torch.cuda.synchronize()
    for name, cols in (("dy", MF_D), ("h13", 2 * MF_H), ("dh", 2 * MF_H), ("dx", MF_D)):
        assert nan_count(bufs[name]) == 2 * SLACK * cols, name          # results without a NaN, the rows around them untouched
    dh_ref = K.gemm_nt_dswiglu(dy, w2t, h13)
    assert torch.equal(dh, dh_ref), int((dh != dh_ref).any(1).nonzero()[0])
    dx_ref = K.gemm_nt(dh_ref, w13t)
    assert torch.equal(dx, dx_ref), int((dx != dx_ref).any(1).nonzero()[0])
    del dh_ref, dx_ref
    cross = 2 ** 31 // (2 * MF_H * 2)                                    # 349 525: the first row whose byte offset has bit 31 set
    for lo in (0, cross // 4096 * 4096, M - 4096):
        _check_mlp_rows(lo, lo + 4096, dy, w2t, h13, w13t, dh, dx)


def test_mlp_bwd_fused_refuses_offsets_past_4gib(K):
    """M * ldh * 2 >= 2^32: refused on the host.  Buffers of the real size, so that a missing check could not become a stray write."""
    from frankenstein_amd._lib import FrankenHipError
    M = 700032
    assert M * 2 * MF_H * 2 >= 2 ** 32 and M % 128 == 0
    dy = torch.zeros(M, MF_D, dtype=BF16, device="cuda")
    h13 = torch.zeros(M, 2 * MF_H, dtype=BF16, device="cuda")
    w2t = torch.zeros(MF_H, MF_D, dtype=BF16, device="cuda")
    w13t = torch.zeros(MF_D, 2 * MF_H, dtype=BF16, device="cuda")
    with pytest.raises(FrankenHipError, match="32-bit byte offsets"):
        K.mlp_bwd_fused(dy, w2t, h13, w13t)


@pytest.mark.parametrize("M", [700032, 393216])
def test_mlp_module_routing_at_the_32_bit_limit(K, M):
    """engine.MlpBranch mirrors the kernel's limit (rows * 2H * 2 < 2^32): the SwiGLU MLP alone (models.brainformer.MLP, d = 384, hidden 1536,
    bf16 mode), forward + backward.  700 032 rows must go through fk_gemm_nt_dswiglu + fk_gemm_nt, 393 216 rows through fk_mlp_bwd_fused
    (kernels.TIMERS records the entry points that ran); the input gradient on sampled blocks of rows meets the float64 chain (atol 3e-2,
    rtol 2e-2, as the kernel-level test)."""
    import frankenstein_amd as fa
    from frankenstein_amd.models import brainformer as bf
    cfg = bf.MAEConfig(window_size=8, n_electrodes=8, patch_size=4, dim=MF_D, n_layers=1, head_dim=64, hidden_dim=MF_H, n_heads=6, n_kv_heads=6)
    torch.manual_seed(5)
    mlp = bf.MLP(cfg).cuda()
    gen = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, MF_D, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    dy = (torch.randn(M, MF_D, device="cuda", generator=gen) * 4.0).bfloat16()          # |dx| ~ 0.5 with nn.Linear's default weights
    fa.set_compute_dtype("bf16")
    K.TIMERS = {}
    try:
        y = mlp(x)
        y.backward(dy)
        torch.cuda.synchronize()
        ran = sorted(K.TIMERS)
    finally:
        K.TIMERS = None
    fused = any(n.startswith("mlp_bwd_fused:") for n in ran)
    two = any(n.startswith("gemm_nt_dswiglu:") for n in ran)
    assert (fused, two) == ((False, True) if M * 2 * MF_H * 2 >= 2 ** 32 else (True, False)), ran
    w1, w2, w3 = (w.detach().bfloat16().double().cpu() for w in (mlp.w1.weight, mlp.w2.weight, mlp.w3.weight))
    cross = 2 ** 31 // (2 * MF_H * 2)
    for lo in (cross - 1024, M - 2048):
        xs, ds = x.detach()[lo:lo + 2048].double().cpu(), dy[lo:lo + 2048].double().cpu()
        h1, h3 = xs @ w1.t(), xs @ w3.t()
        sg = torch.sigmoid(h1)
        want_y = (h1 * sg * h3) @ w2.t()
        dg = ds @ w2
        want_dx = (dg * sg * h3 * (1 + h1 * (1 - sg))) @ w1 + (dg * sg * h1) @ w3
        got_y, got_dx = y.detach()[lo:lo + 2048].float().cpu(), x.grad[lo:lo + 2048].float().cpu()
        print(f"M={M} rows {lo}:{lo + 2048}  max |y - f64| = {float((got_y - want_y).abs().max()):.4g}  max |dx - f64| = {float((got_dx - want_dx).abs().max()):.4g}")
        torch.testing.assert_close(got_y, want_y.float(), atol=3e-2, rtol=2e-2)
        torch.testing.assert_close(got_dx, want_dx.float(), atol=3e-2, rtol=2e-2)


# ---- bf16 D = 64 attention, q / k / v / o as column slices of one [1, N, rs] buffer, dq / dk / dv / do of a second one
def _strided_case(K, rs, Nq, Nk, kind, c, prescaled):
    """-> nothing; asserts.  H = 2, D = 64.  Oracle on compact copies (PS_CASES conventions when prescaled), bit-equality with the same call on
    compact tensors, and the NaN count of both big buffers."""
    H, D = 2, 64
    HD, N = H * D, max(Nq, Nk)
    assert rs % 8 == 0 and rs < 2 ** 24 and rs * N < 2 ** 31
    cols = [8000, (rs // 3) // 8 * 8, (2 * rs // 3) // 8 * 8, rs - HD]                     # q, k, v, o  (dq, dk, dv, do): spread over the row
    cq = (1.0 / math.sqrt(D)) * LOG2E
    qc = q(rnd(1, Nq, HD, seed=1) * (cq * 2.0 if prescaled else 1.0), BF16)               # compact CPU copies, bf16-rounded
    kc, vc, doc = q(rnd(1, Nk, HD, seed=2), BF16), q(rnd(1, Nk, HD, seed=3), BF16), q(rnd(1, Nq, HD, seed=4), BF16)
    A = torch.full((1, N, rs), float("nan"), dtype=BF16, device="cuda")
    G = torch.full((1, N, rs), float("nan"), dtype=BF16, device="cuda")
    view = lambda buf, i, n: buf[:, :n, cols[i]:cols[i] + HD].unflatten(-1, (H, D))
    qd, kd, vd, od = view(A, 0, Nq), view(A, 1, Nk), view(A, 2, Nk), view(A, 3, Nq)
    dqd, dkd, dvd, dod = view(G, 0, Nq), view(G, 1, Nk), view(G, 2, Nk), view(G, 3, Nq)
    for dst, src in ((qd, qc), (kd, kc), (vd, vc), (dod, doc)):
        dst.copy_(src.view(dst.shape).to(BF16))
    assert qd.stride(1) == rs and od.stride(1) == rs and dkd.stride(1) == rs
    m = K.Mask(kind, c)
    o, lse = K.attn_fwd(qd, kd, vd, m, out=od, q_prescaled=prescaled)
    K.attn_bwd(qd, kd, vd, od, dod, lse, dqd, dkd, dvd, m, q_prescaled=prescaled)
    torch.cuda.synchronize()
    # nothing but the eight operand / result regions holds a number
    assert nan_count(A) == N * rs - 2 * (Nq + Nk) * HD
    assert nan_count(G) == N * rs - 2 * (Nq + Nk) * HD
    # the oracle
    qr = (qc.view(1, Nq, H, D) / (cq if prescaled else 1.0)).requires_grad_(True)
    kr, vr = kc.view(1, Nk, H, D).clone().requires_grad_(True), vc.view(1, Nk, H, D).clone().requires_grad_(True)
    mt = mask_tensor(kind, c, Nq, Nk)
    oref = ref_attn(qr, kr, vr, mt)
    close(od, oref, BF16, atol16=2e-2)
    s = (qr.transpose(1, 2) @ kr.transpose(1, 2).transpose(-1, -2)) / math.sqrt(D)
    if mt is not None:
        s = s.masked_fill(~mt, float("-inf"))
    torch.testing.assert_close(lse.cpu(), torch.logsumexp(s, -1).detach(), atol=3e-2, rtol=2e-3 if prescaled else 1e-4)
    oref.backward(doc.view(1, Nq, H, D))
    close(dqd, qr.grad, BF16, atol16=4e-2)
    close(dkd, kr.grad, BF16, atol16=4e-2)
    close(dvd, vr.grad, BF16, atol16=4e-2)
    # the same call on compact tensors: the arithmetic does not depend on addresses
    q2, k2, v2, g2 = (dev(t_, BF16).view(1, -1, H, D) for t_ in (qc, kc, vc, doc))
    o2, lse2 = K.attn_fwd(q2, k2, v2, m, q_prescaled=prescaled)
    dq2, dk2, dv2 = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(v2)
    K.attn_bwd(q2, k2, v2, o2, g2, lse2, dq2, dk2, dv2, m, q_prescaled=prescaled)
    for name, a, b in (("o", od, o2), ("lse", lse, lse2), ("dq", dqd, dq2), ("dk", dkd, dk2), ("dv", dvd, dv2)):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))


STRIDE_CASES = [
    # Nq, Nk, kind, c, prescaled                     which loader it selects
    (333, 333, 1, 0, False),                       # the classic kernels (dma_tile_bf16_d64 / DmaCursor), causal and ragged
    (448, 128, 0, 0, True),                        # the generated dK/dV stream
    (128, 320, 0, 0, True),                        # the generated dQ stream
    (256, 384, 0, 0, True),                        # the generated forward stream
    (512, 512, 2, 128, True),                      # block-causal, 128-key blocks: the last rows lie 3.9 GiB from the base
    (256, 256, 0, 0, True),                        # the wide dK/dV stream (256-key blocks, the benchmark's)
    (333, 333, 1, 0, True),                        # the pre-scaled kernels' own loops (dma_group_bf16_d64, DmaCursor), causal and ragged
]


@pytest.mark.parametrize("case", STRIDE_CASES)
def test_attention_d64_large_row_stride(K, case):
    """row stride 4 100 000 elements: at 512 rows the head slab is 2.1e9 elements (< 2^31) and the 32-bit byte offsets of the LDS-DMA loaders
    and the generated streams (__umul24(row, rs) * 2) reach 3.9 GiB"""
    _strided_case(K, 4_100_000, *case)


@pytest.mark.parametrize("kind", [0, 1])
def test_attention_d64_largest_24_bit_stride(K, kind):
    """row stride 2^24 - 8, the largest legal operand of the 24-bit multiply, with 120 rows (rs * N < 2^31)"""
    _strided_case(K, 2 ** 24 - 8, 120, 120, kind, 0, False)
    _strided_case(K, 2 ** 24 - 8, 120, 120, kind, 0, True)
    if kind == 0:
        _strided_case(K, 2 ** 24 - 8, 128, 128, 0, 0, True)               # whole tiles: the generated streams (rs * N = 2^31 - 1024)


def test_attention_d64_large_row_stride_few_queries(K):
    """the key-splitting kernels of the perceiver read-out shape (Nq <= 32, Nk >= 1024) use the same loader: 1040 keys at a row stride of
    2 000 000 elements (slab 2.08e9 < 2^31, last key rows 3.9 GiB from the base)"""
    _strided_case(K, 2_000_000, 32, 1040, 0, 0, False)


def test_attention_d64_stride_limits_are_refused(K):
    """just outside: a row stride of 2^24 (8 rows, really allocated) and a head slab of exactly 2^31 elements"""
    from frankenstein_amd._lib import FrankenHipError
    H, D = 2, 64
    for rs, N in ((2 ** 24, 8), (2 ** 23, 256)):
        A = torch.zeros((1, N, rs), dtype=BF16, device="cuda")
        G = torch.zeros((1, N, rs), dtype=BF16, device="cuda")
        v = lambda buf, i: buf[:, :, i * 4096:i * 4096 + H * D].unflatten(-1, (H, D))
        with pytest.raises(FrankenHipError, match="row strides < 2\\^24"):
            K.attn_fwd(v(A, 0), v(A, 1), v(A, 2), out=v(A, 3))
        with pytest.raises(FrankenHipError, match="row strides < 2\\^24"):
            K.attn_bwd(v(A, 0), v(A, 1), v(A, 2), v(A, 3), v(G, 3), torch.zeros(1, H, N, device="cuda"), v(G, 0), v(G, 1), v(G, 2))
        assert float(A.abs().max()) == 0.0 and float(G.abs().max()) == 0.0
        del A, G


# =============================================================================================== C. decode kernels
DECODE_POS = [0, 1, 63, 64, 255, 256, 700, 1023]
TMAX = 1025                                             # one spare row: even an off-by-one build stays inside the cache


def _decode_ref(qkv, kv, pos, H, D):
    """float64 softmax attention of q = qkv[:, :d] over cache rows 0..pos -> [B, d]"""
    B, d = qkv.shape[0], H * D
    qh = qkv[:, :d].double().view(B, H, 1, D)
    kh = kv[:, :pos + 1, :d].double().view(B, pos + 1, H, D).transpose(1, 2)
    vh = kv[:, :pos + 1, d:].double().view(B, pos + 1, H, D).transpose(1, 2)
    p = torch.softmax((qh @ kh.transpose(-1, -2)) / math.sqrt(D), -1)
    return (p @ vh).view(B, d)


def _decode_case(K, dtype, D, pos, spike=None):
    B, H = 3, (1 if D == 128 else 2)
    d = H * D
    qkv = q(rnd(B, 3 * d, seed=pos + 1), dtype)
    kv = rnd(B, TMAX, 2 * d, seed=pos + 2)
    if spike is not None:
        kv[:, spike, :d] *= 6.0                                             # a late key far above the running maximum of its thread and wave
    kv = q(kv, dtype)
    kv[:, pos + 1:] = float("nan")                                          # one key too many poisons the output
    got = K.attn_decode(dev(qkv, dtype), dev(kv, dtype), torch.tensor([pos], dtype=torch.int32, device="cuda"), H)
    want = _decode_ref(qkv, kv, pos, H, D)
    err = float((got.double().cpu() - want).abs().max())
    print(f"attn_decode D={D} {dtype} pos={pos} spike={spike}: max |o - f64| = {err:.3g}")
    close(got, want, dtype, **({} if dtype == torch.float32 else {"atol16": 2e-2}))


@pytest.mark.parametrize("dtype", TK.DT)
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_attn_decode_against_float64_softmax(K, dtype, D):
    """fk_attn_decode, q read from a [B, 3d] qkv row (q_bs = 3d), cache [B, 1025, 2d] with NaN behind row pos: one key (pos 0), a partial
    wave, exactly one / four waves, threads with one, two and four loop trips.  close() defaults in fp32 (2e-5), the forward-attention
    atol 2e-2 in bf16."""
    for pos in DECODE_POS:
        _decode_case(K, dtype, D, pos)


@pytest.mark.parametrize("dtype", TK.DT)
@pytest.mark.parametrize("pos,spike", [(255, 200), (700, 300), (1023, 700)])
def test_attn_decode_rescales_running_maxima(K, dtype, pos, spike):
    """a key scaled by 6 late in the cache: in the last wave of a one-trip launch (200), in a thread's second trip (300: the in-thread
    rescale a = exp(m - mn) with a finite m) and its third (700) — the per-thread, per-wave and block-wide merges all see unequal maxima"""
    _decode_case(K, dtype, 64, pos, spike)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("dtype", TK.DT)
@pytest.mark.parametrize("last", [False, True])
def test_kv_append_writes_exactly_one_row(K, dtype, last):
    B, d, tmax = 3, 96, 40
    pos = tmax - 1 if last else 0
    big = (torch.arange((B + 2) * tmax * 2 * d, dtype=torch.float32) % 251 - 125).view(B + 2, tmax, 2 * d).to(dtype).cuda()   # a sample of slack on both sides
    before = big.clone()
    qkv = dev(rnd(B, 3 * d, seed=3), dtype)
    K.kv_append_(qkv, big[1:B + 1], torch.tensor([pos], dtype=torch.int32, device="cuda"))
    want = before.clone()
    want[1:B + 1, pos] = qkv[:, d:]
    assert torch.equal(_bits(big), _bits(want))
    assert not torch.equal(_bits(big), _bits(before))


@pytest.mark.parametrize("dtype", TK.DT)
def test_gpt_embed_step_first_and_last_position(K, dtype):
    B, d, V, block = 4, 80, 211, 1024
    wte, wpe = rnd(V, d, seed=1), rnd(block, d, seed=2)
    idx = torch.tensor([0, V - 1, 17, 100])
    for pos in (0, block - 1):
        got = K.gpt_embed_step(dev(idx), dev(wte), dev(wpe), torch.tensor([pos], dtype=torch.int32, device="cuda"), dtype)
        want = (wte[idx] + wpe[pos]).to(dtype)                              # one fp32 add, one rounding
        assert torch.equal(_bits(got.cpu()), _bits(want)), pos


@pytest.mark.parametrize("dtype", TK.DT)
def test_decode_chain_equals_causal_attention(K, dtype):
    """fk_gpt_embed_step -> fk_kv_append -> fk_attn_decode over 300 steps, the position advanced on the device by fk_sample_topk's
    pos_inc (as GPT.generate's captured graph does): the 300 outputs equal attn_fwd with a causal mask over the same tokens, row by row.
    The embedding table is 3d wide, so the embedding row IS the q|k|v row and no other kernel takes part."""
    B, H, D, V, steps = 2, 2, 64, 50, 300
    d = H * D
    wte, wpe = rnd(V, 3 * d, seed=1), rnd(steps, 3 * d, seed=2, scale=0.5)
    idx = torch.randint(0, V, (B, steps), generator=torch.Generator().manual_seed(3)).cuda()
    kv = torch.full((B, steps + 1, 2 * d), float("nan"), dtype=dtype, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    state = K.SampleState("cuda", seed=1)
    logits = torch.zeros(B, 8, device="cuda")
    qkv_all = torch.empty(B, steps, 3 * d, dtype=dtype, device="cuda")
    o_all = torch.empty(B, steps, d, dtype=dtype, device="cuda")
    wted, wped = dev(wte), dev(wpe)
    for t in range(steps):
        qkv = K.gpt_embed_step(idx[:, t].contiguous(), wted, wped, pos, dtype)
        K.kv_append_(qkv, kv, pos)
        o_all[:, t] = K.attn_decode(qkv, kv, pos, H)
        qkv_all[:, t] = qkv
        K.sample_topk(logits, 1.0, None, state, pos_inc=pos)
    assert int(pos) == steps
    want_qkv = (wte[idx.cpu()] + wpe[None]).to(dtype)
    assert torch.equal(_bits(qkv_all.cpu()), _bits(want_qkv))
    assert torch.equal(_bits(kv[:, :steps]), _bits(qkv_all[..., d:])) and nan_count(kv) == B * 2 * d
    qh, kh, vh = (qkv_all[..., i * d:(i + 1) * d].unflatten(-1, (H, D)) for i in range(3))
    o, _ = K.attn_fwd(qh, kh, vh, K.Mask(K.MASK_CAUSAL))
    close(o_all.view(B, steps, H, D), o, dtype, **({} if dtype == torch.float32 else {"atol16": 2e-2}))
    f = lambda t_: t_.float().cpu()
    close(o_all.view(B, steps, H, D), ref_attn(f(qh), f(kh), f(vh), mask_tensor(1, 0, steps, steps)), dtype, **({} if dtype == torch.float32 else {"atol16": 2e-2}))


# =============================================================================================== D. the fast paths' argument checks
def test_fast_paths_leave_bad_arguments_to_launch_nt(K):
    """fk_gemm_nt_rope / fk_gemm_nt_swiglu at a row count that takes the token-on-the-lane kernels (49 152), with an empty problem and with
    leading dimensions shorter than their rows: the error launch_nt gives, and not a byte of the output changed.  The kernels get an
    interior pointer of a larger buffer (more than a row of slack on both sides), so whatever a build without the checks would write
    lands inside it and shows up as a changed byte."""
    from frankenstein_amd import _lib
    M, d, D, Hh, Hm = 49152, 384, 64, 6, 1536
    N = 3 * Hh * D
    x = torch.zeros(M, d, dtype=BF16, device="cuda")
    st = K._stream()
    bf = K.fk_dtype(x)
    # --- the q|k|v projection with RoPE
    w = torch.zeros(N, d, dtype=BF16, device="cuda")
    ang = R.rope_angles(D, 64, 10000.0)
    table = dev(torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous())
    T = 64
    slack = 4 * N
    buf = torch.full((M * N + 2 * slack,), 3.0, dtype=BF16, device="cuda")
    out = buf[slack:]
    rope = lambda n, ldc: _lib.lib().fk_gemm_nt_rope(x.data_ptr(), d, w.data_ptr(), d, out.data_ptr(), ldc, M, n, d, None, table.data_ptr(), 0, T, 0, D,
                                                     min(2 * Hh * D, n), 0, 0, bf, st)
    for n, ldc, what in ((0, N, "empty problem"), (N, N - 8, "leading dimensions")):
        with pytest.raises(_lib.FrankenHipError, match=what):
            _lib.check(rope(n, ldc), "fk_gemm_nt_rope")
        torch.cuda.synchronize()
        assert bool((buf == 3.0).all()), (n, ldc)
    assert rope(N, N) == 0                                                 # and the legal call runs (zeros in, zeros out)
    assert float(out[:M * N].abs().max()) == 0.0 and bool((buf[:slack] == 3.0).all()) and bool((buf[slack + M * N:] == 3.0).all())
    del buf, out
    # --- the SwiGLU up-projection
    w13 = torch.zeros(2 * Hm, d, dtype=BF16, device="cuda")
    slack = 4 * 2 * Hm
    hbuf = torch.full((M * 2 * Hm + 2 * slack,), 3.0, dtype=BF16, device="cuda")
    gbuf = torch.full((M * Hm + 2 * slack,), 3.0, dtype=BF16, device="cuda")
    h13, g = hbuf[slack:], gbuf[slack:]
    up = lambda h, ldh, ldg: _lib.lib().fk_gemm_nt_swiglu(x.data_ptr(), d, w13.data_ptr(), d, h13.data_ptr(), ldh, g.data_ptr(), ldg, M, h, d, bf, st)
    for h, ldh, ldg, what in ((0, 2 * Hm, Hm, "hidden size"), (Hm, 2 * Hm - 8, Hm, "leading dimensions"), (Hm, 2 * Hm, Hm - 8, "leading dimensions")):
        with pytest.raises(_lib.FrankenHipError, match=what):
            _lib.check(up(h, ldh, ldg), "fk_gemm_nt_swiglu")
        torch.cuda.synchronize()
        assert bool((hbuf == 3.0).all()) and bool((gbuf == 3.0).all()), (h, ldh, ldg)
    assert up(Hm, 2 * Hm, Hm) == 0
    assert float(h13[:M * 2 * Hm].abs().max()) == 0.0 and float(g[:M * Hm].abs().max()) == 0.0
    for b_, n_ in ((hbuf, M * 2 * Hm), (gbuf, M * Hm)):
        assert bool((b_[:slack] == 3.0).all()) and bool((b_[slack + n_:] == 3.0).all())
