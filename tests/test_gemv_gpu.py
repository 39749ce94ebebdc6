"""fk_gemv_nt on the MI355X: the weight-streaming skinny product of the decode step (1 <= M <= 16),
C = act(LN(A) W^T + bias) + residual, against exact integer results and a float64 oracle of the whole chain computed from the
stored (rounded) inputs, plus the properties the decode paths rely on: batch invariance to the bit, strided views, the envelope,
graph capture."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
MS = [1, 2, 3, 5, 8, 16]
# (N, K, rows of the weight buffer): the four layer shapes of GPT-2 124M, its head on the 16-byte-padded shadow, two small ones
SHAPES = [(2304, 768, 2304), (768, 768, 768), (3072, 768, 3072), (768, 3072, 768), (50257, 768, 50264), (211, 64, 211), (1, 8, 1)]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def dev(t, dtype=None):
    t = t.to("cuda")
    return t.to(dtype) if dtype is not None else t


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, want, dtype, atol32=2e-5, rtol32=2e-5, rtol16=2e-2):
    """the tolerances tests/test_kernels_gpu.py::close holds fk_gemm_nt to"""
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    print(f"max |got - want| = {float((got - want).abs().max()):.3e}, |want| max = {float(want.abs().max()):.3e}")
    if dtype == torch.float32:
        torch.testing.assert_close(got, want, atol=atol32, rtol=rtol32)
    else:
        torch.testing.assert_close(got, want, atol=2e-2 * max(1.0, float(want.abs().max())), rtol=rtol16)


def oracle(a, w, bias=None, res=None, ln=None, gelu=False):
    """float64 chain from the values the kernel is given (a, w, bias, res already rounded to the compute dtype; gamma / beta fp32)"""
    x = a.double()
    if ln is not None:
        gamma, beta, eps = ln
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        x = (x - mu) / torch.sqrt(var + eps) * gamma.double()
        if beta is not None:
            x = x + beta.double()
    y = x @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    if gelu:
        y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    if res is not None:
        y = y + res.double()
    return y


# ----------------------------------------------------------------------------------------------- exact integers
@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("M", MS)
def test_gemv_nt_exact_integers(K, dtype, shape, M):
    # asymmetric small-integer operands: every product and partial sum is exact in both dtypes (|sum| <= 9 K + 8 < 2^24), so any lane / column /
    # row mix-up or a dropped K piece changes the result; the rows of the buffer past N hold NaN and must not be read
    N, Kd, rows = shape
    gi = lambda lo, hi, shp, seed: torch.randint(lo, hi, shp, generator=torch.Generator().manual_seed(seed)).float()
    a, w = gi(-3, 4, (M, Kd), 1), gi(-3, 4, (N, Kd), 2)
    w[:, 0] += torch.arange(N) % 5
    bias, res = gi(-4, 5, (N,), 3), gi(-4, 5, (M, N), 4)
    wbuf = torch.full((rows, Kd), float("nan"))
    wbuf[:N] = w
    want = a @ w.t()
    wd = dev(wbuf, dtype)
    got = K.gemv_nt(dev(a, dtype), wd, out_dtype=torch.float32, n=N)
    assert got.shape == (M, N) and torch.equal(got.cpu(), want)
    got = K.gemv_nt(dev(a, dtype), wd, bias=dev(bias, dtype), residual=dev(res, dtype), out_dtype=torch.float32, n=N)
    assert torch.equal(got.cpu(), want + bias + res)


# ----------------------------------------------------------------------------------------------- random data, float64 oracle
CHAINS = {
    "plain": dict(),
    "bias": dict(bias=True),
    "bias+res": dict(bias=True, res=True),
    "ln+bias": dict(ln="beta", bias=True),
    "ln-nobeta": dict(ln="nobeta"),
    "ln+bias+gelu": dict(ln="beta", bias=True, gelu=True),
    "gelu+res": dict(gelu=True, res=True),
    "ln+f32out": dict(ln="beta", f32out=True),
    "all": dict(ln="beta", bias=True, gelu=True, res=True, f32out=True),
}


# every chain at the layer shapes; the 77-MB head at the chains the decode step runs there (plain, LayerNorm + fp32 logits) and the full one
CHAIN_CASES = [(s, c) for s in [(2304, 768), (768, 3072), (211, 64)] for c in sorted(CHAINS)] + \
              [((50257, 768), c) for c in ("plain", "ln+f32out", "all")]


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda sc: f"{sc[0][0]}x{sc[0][1]}-{sc[1]}")
def test_gemv_nt_matches_float64_chain(K, dtype, M, case):
    (N, Kd), chain = case
    c = CHAINS[chain]
    q = lambda t: t.to(dtype).float()
    a = q(rnd(M, Kd, seed=1) * (2.0 if c.get("ln") else 1.0) + (0.5 if c.get("ln") else 0.0))
    w = q(rnd(N, Kd, seed=2, scale=1 / math.sqrt(Kd)))
    bias = q(rnd(N, seed=3)) if c.get("bias") else None
    res = q(rnd(M, N, seed=4)) if c.get("res") else None
    ln = None
    if c.get("ln"):
        ln = (1.0 + 0.1 * rnd(Kd, seed=5), 0.1 * rnd(Kd, seed=6) if c["ln"] == "beta" else None, 1e-5)
    want = oracle(a, w, bias, res, ln, c.get("gelu", False))
    got = K.gemv_nt(dev(a, dtype), dev(w, dtype), bias=None if bias is None else dev(bias, dtype),
                    residual=None if res is None else dev(res, dtype),
                    ln=None if ln is None else (dev(ln[0]), None if ln[1] is None else dev(ln[1]), ln[2]),
                    act="gelu" if c.get("gelu") else None, out_dtype=torch.float32 if c.get("f32out") else None)
    assert got.dtype == (torch.float32 if c.get("f32out") else dtype)
    # fk_gemm_nt's tolerances, unchanged: fp32 atol = rtol = 2e-5 at O(1) outputs, bf16 2e-2 * max(1, |want| max) / rtol 2e-2.  (With fp32 output
    # the bf16 case has no output rounding at all and sits far inside its bound.)
    close(got, want, dtype)


# ----------------------------------------------------------------------------------------------- batch invariance
@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3072, 768), (768, 3072), (2304, 768), (50257, 768), (211, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gemv_nt_rows_do_not_depend_on_the_batch(K, dtype, shape):
    """row m of an M = 16 call == the M = 1 call on that row, bit for bit, with the LayerNorm and the GELU on (the M = 16 launch also groups
    the columns differently from the M = 1 one at these N); the other row buckets (M = 2, 3, 5, 8) agree as well.  Compared on the fp32
    output of the plain product first, i.e. on the accumulators themselves: a bf16 output would hide sums that differ in their last bits
    unless they straddle a rounding boundary."""
    N, Kd = shape
    a = dev(rnd(16, Kd, seed=1) * 2.0 + 0.5, dtype)
    w = dev(rnd(N, Kd, seed=2, scale=1 / math.sqrt(Kd)), dtype)
    bias, res = dev(rnd(N, seed=3), dtype), dev(rnd(16, N, seed=4), dtype)
    ln = (dev(1.0 + 0.1 * rnd(Kd, seed=5)), dev(0.1 * rnd(Kd, seed=6)), 1e-5)
    runs = {
        "accumulators": lambda lo, hi: K.gemv_nt(a[lo:hi], w, out_dtype=torch.float32),
        "ln accumulators": lambda lo, hi: K.gemv_nt(a[lo:hi], w, ln=ln, out_dtype=torch.float32),
        "full chain fp32 out": lambda lo, hi: K.gemv_nt(a[lo:hi], w, bias=bias, residual=res[lo:hi], ln=ln, act="gelu", out_dtype=torch.float32),
        "full chain": lambda lo, hi: K.gemv_nt(a[lo:hi], w, bias=bias, residual=res[lo:hi], ln=ln, act="gelu"),
    }
    for name, run in runs.items():
        full = run(0, 16)
        assert bool(torch.isfinite(full.float()).all()), name
        for m in range(16):
            assert torch.equal(run(m, m + 1), full[m:m + 1]), (name, m)
        for lo, hi in ((0, 2), (2, 5), (0, 5), (5, 8), (0, 8), (8, 16), (3, 12)):
            assert torch.equal(run(lo, hi), full[lo:hi]), (name, lo, hi)


# ----------------------------------------------------------------------------------------------- strided views
@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_gemv_nt_strided_views(K, dtype, M):
    """lda > K, ldc > N, ldr > N: the result lands in the view only, rows and columns around it keep their bits"""
    N, Kd = 211, 128
    big = dev(rnd(M, 3 * Kd, seed=1), dtype)
    a = big[:, Kd:2 * Kd]
    w = dev(rnd(N, Kd, seed=2, scale=1 / math.sqrt(Kd)), dtype)
    rbig = dev(rnd(M, N + 9, seed=3), dtype)
    res = rbig[:, 4:4 + N]
    out = torch.zeros(M + 2, N + 13, device="cuda", dtype=dtype)
    view = out[1:M + 1, 7:7 + N]
    K.gemv_nt(a, w, residual=res, out=view)
    close(view, oracle(a.float().cpu(), w.float().cpu(), res=res.float().cpu()), dtype)
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[1:M + 1, 7:7 + N] = False
    assert float(out[mask].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------- envelope
def test_gemv_nt_refuses_what_is_outside_its_envelope(K):
    from frankenstein_amd._lib import FrankenHipError
    bf = torch.bfloat16
    w = dev(rnd(64, 64, seed=2), bf)
    for M in (0, 17):
        with pytest.raises(FrankenHipError, match="outside 1..16"):
            K.gemv_nt(torch.zeros(M, 64, device="cuda", dtype=bf), w)
    with pytest.raises(FrankenHipError, match="multiple of 8"):        # K = 12 in bf16: not a whole number of 16-byte pieces
        K.gemv_nt(dev(rnd(2, 12, seed=1), bf), dev(rnd(64, 12, seed=2), bf))
    flat = dev(rnd(64 * 65 + 8, seed=3), bf)
    with pytest.raises(FrankenHipError, match="16-byte aligned"):      # W two bytes off a 16-byte boundary
        K.gemv_nt(dev(rnd(2, 64, seed=1), bf), flat[1:1 + 64 * 64].view(64, 64))
    with pytest.raises(FrankenHipError, match="16-byte aligned"):      # rows of W not a multiple of 16 bytes apart
        K.gemv_nt(dev(rnd(2, 64, seed=1), bf), flat[: 64 * 65].view(64, 65)[:, :64])
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
def test_gemv_nt_captured_replay_gives_the_eager_bits(K, dtype):
    M, N, Kd = 3, 2304, 768
    a = dev(rnd(M, Kd, seed=1) * 2.0 + 0.5, dtype)
    w = dev(rnd(N, Kd, seed=2, scale=1 / math.sqrt(Kd)), dtype)
    bias = dev(rnd(N, seed=3), dtype)
    ln = (dev(1.0 + 0.1 * rnd(Kd, seed=5)), dev(0.1 * rnd(Kd, seed=6)), 1e-5)
    eager = K.gemv_nt(a, w, bias=bias, ln=ln, act="gelu")
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.gemv_nt(a, w, bias=bias, ln=ln, act="gelu", out=out)        # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            K.gemv_nt(a, w, bias=bias, ln=ln, act="gelu", out=out)
        for _ in range(3):
            out.zero_()
            graph.replay()
            side.synchronize()
            assert torch.equal(out, eager)
    torch.cuda.current_stream().wait_stream(side)
