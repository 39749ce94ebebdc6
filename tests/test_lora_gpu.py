"""fk_lora_fwd / fk_lora_wgrad / fk_lora_merge (csrc/lora.hip) against the float64 restatement of tests/lora_ref.py, in the idiom of
tests/test_gemm_routes_gpu.py.

Exact operands.  Small integers with an asymmetric ramp in one column of each operand (a fragment, tile, row or k-slot mix-up is a hard
mismatch), x a view with row stride K + 8, A sparse and scaled by a power of two so that u = x A^T (and du in the transposed-role call)
is exactly representable in the compute dtype: asserted on the CPU before the launch.  Every product and sum is then exact in fp32, so
  * u_out and fp32 outputs are BIT-EQUAL to the float64 result, bf16 outputs to its single rounding;
  * fk_lora_fwd over M in {1, 57, 33 = one 32-row tile + 1}, K in {8, 768}, N in {8, 72, 2304 with q_cols = 768, q_scale = 2^-3},
    r in {4, 12, 16, 64}, res absent / separate (out a view inside a sentinel-filled buffer that must come back untouched) / in place,
    both dtypes; and the transposed-role call  lora_fwd(dy, B^T, A^T, res = dh, out = dh)  against the restatement's du and dx;
  * fk_lora_wgrad over M in {1, 63, 67 = one 64-row slice + 3, 192 = three slices}, N = 72, K in {8, 3072}, r in {4, 12, 16, 64}, into
    fresh and into pre-filled integer dA / dB; two calls are torch.equal;
  * fk_lora_merge: the bf16 output has the bits of casting the fp32 output, which is bit-equal to float64 on exact operands.
Random normal operands, every kernel, both dtypes: the error against float64 is at most 4 x the largest error of the CPU evaluation that
rounds at the same points (lora_ref.rounded_*); prints "FRAC <kernel> <dtype> <tensor> <error / bound>".
Every envelope violation returns FK_EINVAL on the host; nothing here launches on an invalid shape."""
import numpy as np
import pytest
import torch

from tests import lora_ref as LR

pytestmark = pytest.mark.gpu

TDT = LR.TDT
SENTINEL = -7.0
S, QS = 0.5, 2.0 ** -3
_OPS = {}


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def ops(M, N, Kd, r):
    """exact operands of a shape, made once and left unchanged"""
    key = (M, N, Kd, r)
    if key not in _OPS:
        _OPS[key] = LR.exact_operands(M, N, Kd, r, seed=1000 * M + 10 * N + Kd + r)
    return _OPS[key]


def dev(a, dtype, pad=0):
    """a float64 array on the GPU in the compute dtype; pad > 0: as a view with row stride cols + pad"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(TDT[dtype])
    if pad:
        wide = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype)
        wide[:, :t.shape[1]] = t
        return wide.cuda()[:, :t.shape[1]]
    return t.cuda()


def rounded(ref, dtype):
    t = torch.from_numpy(np.ascontiguousarray(ref))
    assert torch.equal(t.float().double(), t), "the reference itself is not an fp32 value"
    return t.float() if dtype == "fp32" else t.float().to(torch.bfloat16).float()


def q_of(N):
    return (768, QS) if N == 2304 else (0, 1.0)


FWD = [(M, Kd, N, r, dt) for M in (1, 57, 33) for Kd in (8, 768) for N in (8, 72, 2304) for r in (4, 12, 16, 64) for dt in ("bf16", "fp32")]


@pytest.mark.parametrize("M,Kd,N,r,dtype", FWD, ids=lambda v: str(v))
def test_fwd_exact(K, M, Kd, N, r, dtype):
    x, A, B, res, _ = ops(M, N, Kd, r)
    q_cols, q_scale = q_of(N)
    assert K.lora_route(M, N, Kd, r, TDT[dtype]) == (0 if r <= 32 else 1)
    u_ref, _ = LR.forward(x, A, B, S)
    assert LR.representable(u_ref, dtype) and all(LR.representable(v, dtype) for v in (x, A, B, res))
    xd, Ad, Bd, resd = dev(x, dtype, pad=8), dev(A, dtype), dev(B, dtype), dev(res, dtype)
    assert xd.stride(0) == Kd + 8
    for mode in ("none", "separate", "inplace"):
        _, ref = LR.forward(x, A, B, S, None if mode == "none" else res, q_cols, q_scale)
        if mode == "inplace":
            out = resd.clone()
            got, u = K.lora_fwd(xd, Ad, Bd, S, res=out, out=out, q_cols=q_cols, q_scale=q_scale)
        else:
            buf = torch.full((M, N + 16), SENTINEL, dtype=TDT[dtype], device="cuda")
            out = buf[:, 8:8 + N]
            got, u = K.lora_fwd(xd, Ad, Bd, S, res=resd if mode == "separate" else None, out=out, q_cols=q_cols, q_scale=q_scale)
            assert bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + N:] == SENTINEL).all()), mode
        assert torch.equal(u.float().cpu(), rounded(u_ref, dtype)), mode
        assert torch.equal(got.float().cpu(), rounded(ref, dtype)), mode


@pytest.mark.parametrize("M,Kd,N,r,dtype", [(M, Kd, N, r, dt) for M in (1, 57, 33) for (Kd, N) in ((8, 72), (768, 2304), (3072, 768))
                                             for r in (4, 16, 64) for dt in ("bf16", "fp32")], ids=lambda v: str(v))
def test_fwd_transposed_role_exact(K, M, Kd, N, r, dtype):
    """the data gradient: x = dy [M, N], A = B^T [r, N] (sparse here, so that du is representable), B = A^T [K, r], res = out = dh"""
    dy, Bt, At, dh, _ = ops(M, Kd, N, r)                    # roles swapped: the "K" of this call is the Linear's N
    du_ref, dx_ref, _, _ = LR.backward(np.zeros((M, Kd)), At.T, Bt.T, S, dy)
    assert LR.representable(du_ref, dtype)
    dhd = dev(dh, dtype)
    got, du = K.lora_fwd(dev(dy, dtype, pad=8), dev(Bt, dtype), dev(At, dtype), S, res=dhd, out=dhd)
    assert got.data_ptr() == dhd.data_ptr()
    assert torch.equal(du.float().cpu(), rounded(du_ref, dtype))
    assert torch.equal(dhd.float().cpu(), rounded(dh + dx_ref, dtype))


WG = [(M, Kd, r, dt) for M in (1, 63, 67, 192) for Kd in (8, 3072) for r in (4, 12, 16, 64) for dt in ("bf16", "fp32")]


@pytest.mark.parametrize("M,Kd,r,dtype", WG, ids=lambda v: str(v))
def test_wgrad_exact(K, M, Kd, r, dtype):
    from frankenstein_amd import _lib
    N = 72
    assert _lib.LORA_WGRAD_ROWS == 64
    g = np.random.default_rng(M * 7 + Kd + r)
    x, _, _, _, dy = ops(M, N, Kd, r)
    u = g.integers(-10, 11, size=(M, r)) / 8.0
    du = g.integers(-10, 11, size=(M, r)) / 4.0
    u[:, 0] += (np.arange(M) % 3) / 8.0
    assert all(LR.representable(v, dtype) for v in (x, dy, u, du))
    dA_ref, dB_ref = S * (du.T @ x), S * (dy.T @ u)
    xd, dyd, ud, dud = (dev(v, dtype) for v in (x, dy, u, du))
    dA, dB = K.lora_wgrad(dyd, ud, dud, xd, S)
    assert torch.equal(dA.cpu(), rounded(dA_ref, "fp32")) and torch.equal(dB.cpu(), rounded(dB_ref, "fp32"))
    dA2, dB2 = K.lora_wgrad(dyd, ud, dud, xd, S)
    assert torch.equal(dA, dA2) and torch.equal(dB, dB2)
    pa = g.integers(-64, 65, size=(r, Kd)).astype(np.float64)
    pb = g.integers(-64, 65, size=(N, r)).astype(np.float64)
    dA3, dB3 = dev(pa, "fp32"), dev(pb, "fp32")
    K.lora_wgrad(dyd, ud, dud, xd, S, dA=dA3, dB=dB3, accumulate=True)
    assert torch.equal(dA3.cpu(), rounded(pa + dA_ref, "fp32")) and torch.equal(dB3.cpu(), rounded(pb + dB_ref, "fp32"))


@pytest.mark.parametrize("N,Kd,r", [(8, 8, 4), (72, 768, 12), (2304, 768, 16), (768, 3072, 64)], ids=lambda v: str(v))
def test_merge_bf16_is_the_cast_of_fp32(K, N, Kd, r):
    _, A, B, _, _ = ops(33, N, Kd, r)
    W = np.random.default_rng(N + Kd).integers(-8, 9, size=(N, Kd)).astype(np.float64)
    Wd, Ad, Bd = dev(W, "fp32"), dev(A, "fp32"), dev(B, "fp32")
    m32 = K.lora_merge(Wd, Ad, Bd, S)
    assert torch.equal(m32.cpu(), rounded(LR.merge(W, A, B, S), "fp32"))
    buf = torch.full((N, Kd + 8), SENTINEL, dtype=torch.bfloat16, device="cuda")
    m16 = K.lora_merge(Wd, Ad, Bd, S, out=buf[:, :Kd])
    assert torch.equal(m16, m32.to(torch.bfloat16)) and bool((buf[:, Kd:] == SENTINEL).all())
    # random masters: still the cast of the fp32 result, bit for bit, and in place on the master
    g = torch.Generator().manual_seed(N)
    Wr, Ar, Br = torch.randn(N, Kd, generator=g).cuda(), torch.randn(r, Kd, generator=g).cuda(), torch.randn(N, r, generator=g).cuda()
    r32 = K.lora_merge(Wr, Ar, Br, 1.7)
    assert torch.equal(K.lora_merge(Wr, Ar, Br, 1.7, out_dtype=torch.bfloat16), r32.to(torch.bfloat16))
    assert torch.equal(K.lora_merge(Wr.clone(), Ar, Br, 1.7, out=None), r32)
    Wc = Wr.clone()
    K.lora_merge(Wc, Ar, Br, 1.7, out=Wc)
    assert torch.equal(Wc, r32)


def frac(name, dtype, tensor, got, ref, cpu):
    """largest error / (4 x the largest error of the CPU evaluation that rounds at the same points)"""
    bound = 4.0 * float(np.max(np.abs(cpu - ref)))
    err = float(np.max(np.abs(got - ref)))
    assert bound > 0.0, "the yardstick is degenerate"
    print(f"FRAC {name} {dtype} {tensor} {err / bound:.3f}  (max err {err:.3e}, bound {bound:.3e})")
    return err <= bound


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("M,N,Kd,r", [(57, 72, 768, 16), (33, 2304, 72, 12), (70, 768, 3072, 64)], ids=lambda v: str(v))
def test_random_operands(K, M, N, Kd, r, dtype):
    g = np.random.default_rng(M + N + Kd + r)
    rt = lambda a: torch.from_numpy(a).to(TDT[dtype]).double().numpy()        # operands ARE compute-dtype values
    x, A, B, res, dy = rt(g.standard_normal((M, Kd))), rt(g.standard_normal((r, Kd)) / np.sqrt(Kd)), rt(g.standard_normal((N, r))), \
        rt(g.standard_normal((M, N))), rt(g.standard_normal((M, N)))
    q_cols, q_scale = q_of(N)
    s = 1.25
    ok = []
    # forward
    u_ref, out_ref = LR.forward(x, A, B, s, res, q_cols, q_scale)
    u_cpu, out_cpu = LR.rounded_forward(x, A, B, s, dtype, res, q_cols, q_scale)
    out, u = K.lora_fwd(dev(x, dtype, pad=8), dev(A, dtype), dev(B, dtype), s, res=dev(res, dtype), q_cols=q_cols, q_scale=q_scale)
    ok.append(frac("fwd", dtype, "u", u.double().cpu().numpy(), u_ref, u_cpu))
    ok.append(frac("fwd", dtype, "out", out.double().cpu().numpy(), out_ref, out_cpu))
    # data gradient: the transposed-role call, in place on dh
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    dh = rt(g.standard_normal((M, Kd)))
    du_ref, dh_ref = LR.forward(dy, Bt, At, s, dh)
    du_cpu, dh_cpu = LR.rounded_forward(dy, Bt, At, s, dtype, dh)
    dhd = dev(dh, dtype)
    _, du = K.lora_fwd(dev(dy, dtype), dev(Bt, dtype), dev(At, dtype), s, res=dhd, out=dhd)
    ok.append(frac("dgrad", dtype, "du", du.double().cpu().numpy(), du_ref, du_cpu))
    ok.append(frac("dgrad", dtype, "dh", dhd.double().cpu().numpy(), dh_ref, dh_cpu))
    # weight gradients from the tensors the launches above stored (compute-dtype u and du are the kernel's operands)
    uq, duq = u.double().cpu().numpy(), du.double().cpu().numpy()
    dA_ref, dB_ref = s * (duq.T @ x), s * (dy.T @ uq)
    dA_cpu, dB_cpu = LR.rounded_wgrad(dy, uq, duq, x, s, dtype)
    dA, dB = K.lora_wgrad(dev(dy, dtype), u, du, dev(x, dtype), s)
    ok.append(frac("wgrad", dtype, "dA", dA.double().cpu().numpy(), dA_ref, dA_cpu))
    ok.append(frac("wgrad", dtype, "dB", dB.double().cpu().numpy(), dB_ref, dB_cpu))
    # merge (fp32 masters whatever the compute dtype)
    W = g.standard_normal((N, Kd)).astype(np.float32).astype(np.float64)
    A32, B32 = A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)
    mg = K.lora_merge(dev(W, "fp32"), dev(A32, "fp32"), dev(B32, "fp32"), s)
    ok.append(frac("merge", dtype, "W", mg.double().cpu().numpy(), LR.merge(W, A32, B32, s), LR.rounded_merge(W, A32, B32, s)))
    assert all(ok), ok


def test_envelope_is_refused_before_any_launch(K):
    from frankenstein_amd import _lib
    lib = _lib.lib()
    t = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    BFd, F32d = _lib.FK_BF16, _lib.FK_F32

    def fwd(M=8, N=8, Kd=8, r=4, dt=BFd, ldx=None, ldo=None, ldr=None, q_cols=0, x=p, res=None, out=p):
        return lib.fk_lora_fwd(x, Kd if ldx is None else ldx, p, p, M, N, Kd, r, 1.0, q_cols, 1.0, res, N if ldr is None else ldr, p, out,
                               N if ldo is None else ldo, dt, None)

    def wg(M=8, N=8, Kd=8, r=4, dt=BFd, ws=None, nb=0):
        return lib.fk_lora_wgrad(p, p, p, p, M, N, Kd, r, 1.0, p, p, 0, dt, ws, nb, None)

    def mg(N=8, Kd=8, r=4, dt=BFd, ldo=None):
        return lib.fk_lora_merge(p, p, p, N, Kd, r, 1.0, p, Kd if ldo is None else ldo, dt, None)

    bad = [dict(r=0), dict(r=2), dict(r=6), dict(r=68), dict(Kd=12), dict(N=4), dict(M=0), dict(dt=7), dict(Kd=6, dt=F32d), dict(N=2, dt=F32d),
           dict(M=1 << 31), dict(N=1 << 31), dict(Kd=1 << 31)]
    for kw in bad:
        assert fwd(**kw) == -1 and b"fk_lora_fwd" in lib.fk_last_error(), kw
        assert wg(**kw) == -1 and b"fk_lora_wgrad" in lib.fk_last_error(), kw
        if "M" not in kw:
            assert mg(**kw) == -1 and b"fk_lora_merge" in lib.fk_last_error(), kw
    for kw in (dict(ldx=0), dict(ldx=12, Kd=8), dict(ldo=4), dict(res=p, ldr=4), dict(q_cols=9), dict(q_cols=-1), dict(x=None), dict(out=None),
               dict(x=p + 2), dict(ldx=1 << 31)):
        assert fwd(**kw) == -1, kw
    assert wg(M=65) == -1 and b"workspace" in lib.fk_last_error()                      # two slices need the workspace
    assert wg(M=65, ws=p, nb=lib.fk_lora_wgrad_workspace_bytes(65, 8, 8, 4) - 4) == -1
    assert mg(ldo=4) == -1 and mg(ldo=10) == -1
    assert lib.fk_lora_wgrad_workspace_bytes(64, 8, 8, 4) == 0 and lib.fk_lora_wgrad_workspace_bytes(65, 8, 8, 4) == 2 * (8 * 4 + 4 * 8) * 4
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0                                                 # nothing was written
