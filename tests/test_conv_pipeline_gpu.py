"""Every path of the tokenizer's convolution helpers (csrc/conv.hip) and of the device input pipeline (csrc/pipeline.hip) on the MI355X.
im2col / col2im run on small integers and must be bit-equal to an explicit unfold and to its float64 adjoint (index_add_ over the same
index map), every element; ELU against float64; argmax on planted ties; the pipeline against the float64 numpy restatement of
tests/pipeline_ref.py (held to scipy by tests/test_pipeline_ref_cpu.py).

    branch or limit                                              source                                     test
    -----------------------------------------------------------  -----------------------------------------  ---------------------------------------
    Cin = one vector (bf16 8, fp32 4)                            im2col1d_kernel / col2im1d_kernel `cv`     test_im2col / test_col2im (2,11,8,3,1,1), (3,5,4,7,1,9)
    padding 54 > T: every tap but the last is padding            `ts >= 0 && ts < Tin`; `num < 0`                (3,5,4,7,1,9), fp32
    kernel 2 x stride, odd T                                     Tout = (T - 1) / stride + 1                (2,13,24,4,2,1)
    stride > kernel reach: time steps no tap reaches are 0       `num % stride != 0`                        (1,9,16,2,4,1)
    `t >= Tout`                                                  col2im1d_kernel                            (2,13,24,4,2,1), (1,9,16,2,4,1)
    the stem (K = 5)                                             the k loop                                 (2,40,32,5,1,1)
    col2im1d_kernel<bf16> (dcols in the dtype under test)        bf16x8 loads, (bf16_t) stores              test_col2im[bf16]
    the 65 536-block grid cap: the stride loop runs twice        fk_grid(work, 65536)                       test_past_the_grid_cap (im2col, col2im, elu_fwd)
    ELU at 0, -0, +-tiny, denormals, -100, bf16; close() and     elu_fwd_kernel / elu_bwd_kernel            test_elu
      an elementwise bound with one bf16 rounding
    argmax: ld > cols, cols < 64, rows % 4 != 0, a tie of a      argmax_rows_kernel                         test_argmax
      later pass of a lower lane with an earlier pass of a
      higher one (70 / 10), a tie within a lane (c, c + 64),
      a row of -inf, the maximum in the last column
    C > 256: the gridDim.y column loop / second column block     trial_sums_kernel, block_stats_kernel      test_block_stats (C = 260)
    a block without trials: mean 0, std 1                        `n > 0.0`                                  test_block_stats
    a constant channel (0.3), a one-row trial alone in its       `sd == 0.0`                                test_block_stats
      block: std 1
    mean 3000, deviation 0.5                                     fp64 accumulation                          test_block_stats
    Tmax > 64: the `t += gridDim.y` loop; C > 256: the column    zscore_smooth_pad_kernel                   test_zscore_smooth_pad (Tmax 130, C 260)
      loop
    trials of 1, 2, 3, 4 rows: the reflection wraps repeatedly   reflect_idx                                test_zscore_smooth_pad
    trials of Tmax, Tmax + 1, 2 Tmax rows: truncation after      `t < len`                                  test_zscore_smooth_pad
      smoothing; padding rows exactly 0
    sigma 1.1 (other taps); sigma 2.0 refused                    fk_zscore_smooth_pad                       test_zscore_smooth_pad, test_sigma_2_is_refused

The im2col and col2im buffers of test_past_the_grid_cap are larger than the 256 MiB the guard-band allocator of tests/poison.py tracks:
they are allocated normally, and what the calls write is verified in full on the device instead.

Largest |kernel - float64| observed on an MI355X per group, the bound in force in brackets:

    group                                   fp32                         bf16
    --------------------------------------  ---------------------------  ---------------------------
    im2col, col2im (small and past the cap)  bit-equal, as asserted       bit-equal, as asserted
    elu forward / backward                  3.6e-8 / 9.0e-8: 0.001 /     2.0e-3 / 3.7e-3: 0.89 / 0.89 of the elementwise bound
                                              0.003 of the elementwise     2^-8 |ref| + the fp32 bound (one rounding of the output);
                                              bound 2e-5 / 1e-5 + 2e-5     close() of tests/test_kernels_gpu.py allows 0.20 / 0.05
                                              |ref|                        (2e-2 x max(1, |ref|max))
    elu forward past the cap                3.5e-8  (2e-5)
    argmax                                  exact, as asserted           exact, as asserted
    block_stats mean / std                  0.50 / 0.50 ulps (2 ulps): 6.5e-5 at mean 3000, 8.5e-8
    zscore_smooth_pad, sigma 1.0 / 1.1      5.3e-7 / 3.9e-7  (2e-5), |ref|max 3.4"""
import numpy as np
import pytest
import torch

from tests import pipeline_ref as PR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
CAP = 65536 * 256                         # work items one pass of the capped grid covers

#             B,  T, Cin, K, stride, dil
CONV_CASES = [(2, 11, 8, 3, 1, 1), (3, 5, 4, 7, 1, 9), (2, 13, 24, 4, 2, 1), (1, 9, 16, 2, 4, 1), (2, 40, 32, 5, 1, 1)]
CONV_PARAMS = [(c, d) for c in CONV_CASES for d in DT if d == F32 or c[2] % 8 == 0]


def dtid(d):
    return "bf16" if d == BF16 else "fp32"


def pid(v):
    return "-".join(str(i) for i in v) if isinstance(v, tuple) else dtid(v)


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def tap_map(T, K, stride, dil):
    """-> (Tout, src int64 [Tout, K]): the time step of x that tap k of output step t reads, -1 in the causal padding"""
    tout = (T - 1) // stride + 1
    src = torch.arange(tout)[:, None] * stride + torch.arange(K)[None, :] * dil - dil * (K - 1)
    assert int(src.max()) < T
    return tout, torch.where(src >= 0, src, torch.full_like(src, -1))


# ----------------------------------------------------------------------------------------------- im2col / col2im
@pytest.mark.parametrize("case,dtype", CONV_PARAMS, ids=pid)
def test_im2col(K, case, dtype):
    """bit-equal to an explicit left-padded unfold"""
    B, T, C, ks, stride, dil = case
    x = ints((B, T, C), -8, 8, 11 + T)
    pad = dil * (ks - 1)
    tout, src = tap_map(T, ks, stride, dil)
    xp = torch.nn.functional.pad(x, (0, 0, pad, 0))
    ref = torch.stack([torch.cat([xp[:, t * stride + k * dil] for k in range(ks)], -1) for t in range(tout)], 1).reshape(B * tout, ks * C)
    if pad > T:
        assert bool((src[:, :-1] < 0).all()) and not bool(ref.view(B, tout, ks, C)[:, :, :-1].any())      # every tap but the last: padding
    cols = K.im2col1d(x.to(dtype).cuda(), ks, stride, dil)
    assert cols.dtype == dtype and torch.equal(cols.float().cpu(), ref)


@pytest.mark.parametrize("case,dtype", CONV_PARAMS, ids=pid)
def test_col2im(K, case, dtype):
    """dcols in the dtype under test; bit-equal to the float64 adjoint (sums of at most K integers in [-8, 8]: exact in bf16 too), the time
    steps no tap reaches exactly 0"""
    B, T, C, ks, stride, dil = case
    tout, src = tap_map(T, ks, stride, dil)
    g = ints((B, tout, ks, C), -8, 8, 23 + T)
    ref = torch.zeros(B, T, C, dtype=torch.float64)
    live = src >= 0
    ref.index_add_(1, src[live], g.double()[:, live])
    reached = torch.zeros(T, dtype=torch.bool)
    reached[src[live]] = True
    if stride > dil * (ks - 1) + 1:
        assert not bool(reached.all())
    dx = K.col2im1d(g.view(B * tout, ks * C).to(dtype).cuda(), B, T, C, ks, stride, dil)
    assert dx.dtype == dtype and torch.equal(dx.double().cpu(), ref)
    assert not bool(dx[:, ~reached.cuda()].any())


def test_past_the_grid_cap(K):
    """More than 65 536 x 256 work items per call (fp32, one vector per time step), verified on the device with torch indexing."""
    T = CAP // 2 + 300                                             # im2col: T * K work items
    x = torch.randint(-8, 9, (1, T, 4), device="cuda").float()
    cols = K.im2col1d(x, 2, 1, 1).view(T, 2, 4)
    assert 2 * T > CAP
    assert torch.equal(cols[:, 1], x[0]) and torch.equal(cols[1:, 0], x[0, :-1]) and not bool(cols[0, 0].any())
    del cols, x
    T = CAP + 300                                                  # col2im: T work items
    g = torch.randint(-8, 9, (T, 2, 4), device="cuda").float()
    dx = K.col2im1d(g.view(T, 8), 1, T, 4, 2, 1, 1)[0]
    assert torch.equal(dx[:-1], g[:-1, 1] + g[1:, 0]) and torch.equal(dx[-1], g[-1, 1])
    del dx, g
    n = CAP + 771                                                  # elu: n work items
    x = (torch.arange(n, device="cuda") % 1021).float() / 64.0 - 8.0
    y = K.elu_fwd(x)
    want = torch.where(x > 0, x.double(), torch.expm1(x.double()))
    err = float((y.double() - want).abs().max())
    print(f"CONVPIPE elu past the cap: largest error {err:.3e}")
    assert err <= 2e-5 and bool((y[x > 0] == x[x > 0]).all())


# ----------------------------------------------------------------------------------------------- ELU, argmax
def close(got, want, dtype, atol32, tag):
    """close() of tests/test_kernels_gpu.py against a float64 reference"""
    got, want = got.double().cpu(), want.double()
    print(f"CONVPIPE {tag} {dtid(dtype)}: largest error {float((got - want).abs().max()):.3e}")
    if dtype == F32:
        torch.testing.assert_close(got, want, atol=atol32, rtol=2e-5)
    else:
        torch.testing.assert_close(got, want, atol=2e-2 * max(1.0, float(want.abs().max())), rtol=2e-2)
    # every element: the fp32 tolerance, plus one rounding of the output to bf16 (the arithmetic is fp32 in both dtypes) — the form of
    # check_bound in tests/test_gemm_routes_gpu.py; close() above is 100 x looser in bf16 on values below 1
    bound = atol32 + 2e-5 * want.abs() + (2.0 ** -8 * want.abs() if dtype == BF16 else 0.0)
    frac = (got - want).abs() / bound
    print(f"CONVPIPE {tag} {dtid(dtype)}: worst {float(frac.max()):.3f} of the elementwise bound, close() atol {2e-2 * max(1.0, float(want.abs().max())):.3f}")
    assert float(frac.max()) <= 1.0, (tag, int(frac.argmax()), float(got.flatten()[frac.argmax()]), float(want.flatten()[frac.argmax()]))


@pytest.mark.parametrize("dtype", DT, ids=dtid)
def test_elu(K, dtype):
    pts = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-38, -1e-38, 1e-40, -1e-40, 1e-7, -1e-7, -100.0, -20.0, -1.0, 1.0, -0.5, 0.5, 3.0])
    x = torch.cat([pts, torch.randn(1000, generator=torch.Generator().manual_seed(8)) * 3]).to(dtype)
    dy = (torch.randn(x.numel(), generator=torch.Generator().manual_seed(9))).to(dtype)
    x64, dy64 = x.double(), dy.double()
    y = K.elu_fwd(x.cuda())
    close(y, torch.where(x64 > 0, x64, torch.expm1(x64)), dtype, 2e-5, "elu fwd")
    dx = K.elu_bwd(x.cuda(), dy.cuda())
    close(dx, dy64 * torch.where(x64 > 0, torch.ones_like(x64), torch.exp(x64)), dtype, 1e-5, "elu bwd")
    assert float(y[0]) == 0.0 and float(y[1]) == 0.0 and torch.equal(dx[:2].cpu(), dy[:2])       # x = 0: y = 0 and dx = dy, exactly


@pytest.mark.parametrize("dtype", DT, ids=dtid)
def test_argmax(K, dtype):
    inf = float("inf")
    for rows, cols in ((7, 37), (7, 150), (5, 64), (6, 129)):
        a = ints((rows, cols), -50, 50, rows + cols)
        a[1] = -inf                                                # nothing is larger than the start value: 0
        a[2, cols - 1] = 90.0                                      # the maximum in the last column
        if cols > 70:
            a[3, 70] = a[3, 10] = 77.0                             # lane 6's second pass against lane 10's first: 10
            a[4, 5] = a[4, 69] = 77.0                              # both in lane 5: 5
            a[5, 80] = a[5, 16] = a[5, 17] = 77.0
        want = torch.from_numpy(np.argmax(a.numpy(), axis=1))      # the first on ties
        assert int(want[1]) == 0 and int(want[2]) == cols - 1 and (cols <= 70 or (int(want[3]), int(want[4]), int(want[5])) == (10, 5, 16))
        buf = torch.full((rows, cols + 8), 1e9).to(dtype).cuda()   # a view with ld > cols: what lies beside a row is larger than all of it
        buf[:, :cols] = a.to(dtype).cuda()
        idx = K.argmax_rows(buf[:, :cols])
        assert torch.equal(idx.cpu(), want), (rows, cols, idx.cpu().tolist(), want.tolist())


# ----------------------------------------------------------------------------------------------- input pipeline
def ulps32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_block_stats():
    from frankenstein_amd.utils import data_utils as du
    C, nblocks = 260, 5
    rng = np.random.default_rng(41)
    lens = [1, 3, 5, 130, 260, 2, 4, 9, 131, 1]
    blocks = [0, 0, 0, 0, 0, 1, 1, 1, 1, 3]                        # block 2 and block 4 have no trials; block 3 is one row
    trials = [(rng.standard_normal((n, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-1.0, 1.0, C)).astype(np.float32) for n in lens]
    for x in trials:
        x[:, 7] = np.float32(0.3)                                  # constant in every block
        x[:, 258] = np.float32(-2.5)
        x[:, 9] = (3000.0 + 0.5 * rng.standard_normal(x.shape[0])).astype(np.float32)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    xd = torch.from_numpy(np.concatenate(trials)).cuda()
    mean, std = du.block_stats(xd, torch.from_numpy(off).cuda(), torch.tensor(blocks, dtype=torch.int32).cuda(), nblocks)
    mean, std = mean.cpu().numpy().astype(np.float64), std.cpu().numpy().astype(np.float64)
    rm, rs = PR.block_stats(trials, blocks, nblocks)
    for b in (2, 4):
        assert np.array_equal(mean[b], np.zeros(C)) and np.array_equal(std[b], np.ones(C)), f"block {b} has no trials"
    assert np.array_equal(std[3], np.ones(C)) and np.array_equal(mean[3], trials[-1][0].astype(np.float64))
    assert np.array_equal(std[:, 7], np.ones(nblocks)) and np.array_equal(std[:, 258], np.ones(nblocks)), (std[:, 7], std[:, 258])
    assert np.array_equal(mean[:2, 7], np.full(2, np.float64(np.float32(0.3))))
    em, es = np.abs(mean - rm) / ulps32(rm + (rm == 0)), np.abs(std - rs) / ulps32(rs)
    print(f"CONVPIPE block_stats: mean {em.max():.2f} ulps (|error| {np.abs(mean - rm).max():.3e}), std {es.max():.2f} ulps ({np.abs(std - rs).max():.3e}); "
          f"channel 9: {np.abs(mean[:2, 9] - rm[:2, 9]).max():.3e}, {np.abs(std[:2, 9] - rs[:2, 9]).max():.3e}")
    assert em.max() <= 2.0 and es.max() <= 2.0


@pytest.mark.parametrize("sigma", [1.0, 1.1])
def test_zscore_smooth_pad(sigma):
    from frankenstein_amd.utils import data_utils as du
    C, tmax = 260, 130
    rng = np.random.default_rng(43)
    lens = [1, 2, 3, 4, 5, 9, tmax, tmax + 1, 2 * tmax]
    blocks = ["a", "b", "a", "b", "a", "b", "a", "b", "a"]
    scale, shift = rng.uniform(0.5, 2.0, C), rng.uniform(-1.0, 1.0, C)
    trials = [(rng.standard_normal((n, C)) * scale + shift).astype(np.float32) for n in lens]
    out = du.process_and_pad(trials, blocks, max_length=tmax, sigma=sigma)
    assert out.shape == (len(lens), tmax, C) and out.dtype == torch.float32
    got = out.cpu().numpy().astype(np.float64)
    want = PR.process_and_pad(trials, blocks, tmax, sigma)
    for i, n in enumerate(lens):
        assert not got[i, n:].any(), f"trial {i}: the padding rows must be exactly 0"
        assert np.abs(got[i, :min(n, tmax)]).max() > 0.0
    print(f"CONVPIPE zscore_smooth_pad sigma {sigma}: largest error {np.abs(got - want).max():.3e}, |ref|max {np.abs(want).max():.3f}")
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-7)
    if sigma != 1.0:
        assert np.abs(want - PR.process_and_pad(trials, blocks, tmax, 1.0)).max() > 1e-2       # another sigma is another result


def test_sigma_2_is_refused():
    from frankenstein_amd._lib import FrankenHipError
    from frankenstein_amd.utils import data_utils as du
    x = [np.zeros((5, 8), dtype=np.float32)]
    with pytest.raises(FrankenHipError, match="radius-4"):
        du.process_and_pad(x, [0], max_length=8, sigma=2.0)
