"""Every code path of the row-wise kernels (csrc/norm.hip, csrc/loss_optim.hip, csrc/elementwise.hip, fk_colsum in csrc/gemm.hip) on the
MI355X: each dispatch rung, scalar fallback, grid cap / stride loop and flag that tests/test_kernels_gpu.py never enters.  References are
plain torch in float64 on operands already rounded to the compute dtype; sums that can be made exact (small integers) must be bit-equal.

    branch or limit                                          source                                         test
    -------------------------------------------------------  ---------------------------------------------  ------------------------------------------
    norm rungs: bf16 LPR16 x {1,2,3,4}, LPR64 x {2,4};       fk_norm_fwd / fk_norm_bwd dispatch, norm.hip   test_norm_every_rung
      fp32 LPR16 x {2,4,6}, LPR64 x {2,4}; generic above
    a dim that ends inside an iteration (c < dim false)      norm_fwd_fast_kernel, norm_bwd_fused_kernel    test_norm_every_rung (dims 72, 136, ... 1000)
    fewer rows than a wave's row group                       `ok = row < rows`                              test_norm_every_rung (3 rows)
    dres = None, integer dy -> exact dbeta                   norm_bwd_fused_kernel                          test_norm_every_rung
    accumulate = 1                                           norm_bwd_fused_final, norm_bwd_param_final     test_norm_accumulate
    LayerNorm with want_beta = False                         `if (out)` in the final kernels                test_norm_layer_without_dbeta
    gamma / beta not 16-byte aligned -> generic kernels      `done`, `fits` in fk_norm_fwd / fk_norm_bwd    test_norm_misaligned_gamma_beta
    block caps 2048 (fast fwd), 1024 (fused bwd, LPR16),     FK_NF, nbf, nb in norm.hip                     test_norm_grid_wraps
      8192 (generic), nchunks cap 512; the fused bwd's
      stride loop four times under its cap (LPR64)
    null mean for FK_NORM_LAYER                              FK_CHECK_ARG in fk_norm_bwd                    test_norm_bwd_refuses_null_mean
    colsum scalar path (cols, ld, base)                      fk_colsum, colsum_partial_scalar_kernel        test_colsum_exact[scalar-*]
    colsum vector path: second column chunk, partial and     colsum_partial_kernel                          test_colsum_exact[vector-*]
      full (the row's last vector is a chunk's 256th);
      ld > cols; 512-block cap; accumulate                   colsum_blocks, colsum_final_kernel
    L1 / MSE row_weight, forward cap 1024 blocks             l1_partial_kernel, grid_for(n, 1024)           test_l1_mse_forward_exact
    L1 / MSE backward cap 4096 blocks, weighted divisor      l1_bwd_kernel                                  test_l1_mse_backward_past_the_cap
    CE ld / ldd, ignore_index, targets outside [0, V)        ce_row_kernel, ce_bwd_kernel                   test_cross_entropy_strides_and_targets
    CE backward cap 16 384 blocks                            fk_ce_loss_bwd                                 test_cross_entropy_backward_past_the_cap
    fk_ce_chunk_fwd / _finish / _bwd                         ce_chunk_*_kernel                              test_ce_chunked
    AdamW tail only, body wrap (cap 4096), zero_grad on      adamw_kernel                                   test_adamw_small, test_adamw_body_wrap_and_tail
      the tail, weight_decay 0, clip with grad_scale
    V16 / element-wise grid cap 16 384 blocks                grid_for(work, 16384), elementwise.hip         test_*_past_the_cap (swiglu, gelu, add, cast,
      (vector gather: 4096 blocks)                                                                            copy2d, add2d, rope, gather, scatter, embed, dropout)
    fk_add2d on row-strided views                            add2d_kernel                                   test_add2d_strided_views
    fk_cast_pack_rows row map, cap 8192 blocks               cast_pack_kernel                               test_cast_pack_rows
    fk_cast_pack_multi chunk loop past the 8192-block grid   cast_pack_multi_kernel                         test_shadow_refresh_past_the_grid_cap

Tolerances: element-wise outputs, y and dx use close() of tests/test_kernels_gpu.py (fp32 2e-5, bf16 2e-2 x max(1, |ref|max)) or the value
that file already uses for the operation.  Column reductions of random operands (dgamma, random dbeta) are held to 4 x the error of the
same sum done in fp32 by torch on the CPU (floor 1e-5 x |ref|max): the kernel's tree orders the sum differently, nothing more.

Largest |kernel - float64| observed on an MI355X (all 199 cases; the bound in force where it occurred in brackets):

    group                          fp32                       bf16
    -----------------------------  -------------------------  -------------------------
    norm y                         9.5e-7  (1.1e-4)           1.9e-2  (2.4e-1)
    norm mean / rstd               2.4e-7 / 1.2e-7  (4e-5)    (fp32 outputs)
    norm dx                        9.5e-7  (9.2e-5)           1.6e-2  (1.8e-1)
    norm dgamma / dbeta, random    37 and 300 rows: 1.7e-5 (6.3e-4).  131 202 rows x dim 16, integer dy: dgamma 8.7e-4 (1.3e-2: the floor;
                                   5.4 x torch's own fp32 sum error of 1.6e-4).  No column sum came nearer than 0.07 of its bound.
    integer dbeta, colsum, L1/MSE  exact, as asserted
      sums and counts, casts, packs
    L1/MSE loss, dpred             1.2e-7 (3.3e-5), 1.8e-12 (1.1e-9)   dpred 3.0e-8  (2.3e-7)
    CE loss, lse                   9.5e-7 (1.9e-4), 9.5e-7 (2.8e-4)
    CE dlogits                     3.7e-8  (1.0e-4)           1.4e-3  (2.1e-2)
    CE chunked lse, dlogits        4.8e-7 (1.9e-4), 1.1e-8 (5.1e-6)    dlogits 1.1e-4  (2.0e-3)
    AdamW p, m, v                  1.7e-7 (8.1e-6), 2.2e-9 (3.0e-7), 1.9e-8 (7.2e-7)
    swiglu fwd / bwd               9.5e-7 / 9.5e-7  (1.8e-4)  2.1e-2 / 2.6e-2  (3.3e-1)
    gelu fwd / bwd                 4.8e-7 / 4.8e-7  (8.8e-5)  7.8e-3 / 1.3e-2  (1.8e-1)
    add, gpt_embed                 0                          1.6e-2  (1.4e-1)
    rope                           4.8e-7  (9.5e-5)           1.5e-2  (1.0e-1)
    dropout, dropout + residual    4.8e-7, 9.5e-7  (8.5e-6)   1.0e-2 (6.0e-2), 1.6e-2 (1.1e-1)"""
import math

import numpy as np
import pytest
import torch

from oracle import ref_train as RT

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
F32, BF16 = torch.float32, torch.bfloat16
CAP = 16384 * 256                         # work items one pass of a capped element-wise grid covers
WORK = CAP + 771                          # = 5 x 839 015


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


def rint(lo, hi, *shape, seed=0):
    """integer-valued floats in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def drnd(*shape, seed=0, dtype=F32):
    """seeded normal values made on the device (the operands past a grid cap are tens of millions of elements)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda").to(dtype)


def q(t, dtype):
    """round-trip through the compute dtype so the reference sees the same operand values"""
    return t.to(dtype).float().clone()


def close(got, want, dtype, what, atol32=2e-5, rtol32=2e-5, atol16=None, rtol16=2e-2):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    if dtype == torch.float32:
        a, r = atol32, rtol32
    else:
        a, r = (atol16 if atol16 is not None else 2e-2 * max(1.0, float(want.abs().max()))), rtol16
    torch.testing.assert_close(got, want, atol=a, rtol=r, msg=lambda m: f"{what}: {m}")


def check_colsum(got, terms64, what):
    """got [dim] against sum_r terms64[r, :]; bound = 4 x the error of torch's fp32 sum of the same terms on the CPU, floor 1e-5 |ref|max"""
    ref = terms64.sum(0)
    unit = float((terms64.float().sum(0).double() - ref).abs().max())
    bound = max(4.0 * unit, 1e-5 * float(ref.abs().max()))
    err = float((got.detach().double().cpu() - ref).abs().max())
    assert err <= bound, (what, err, bound, unit)


def misaligned(t):
    """a device copy of the fp32 vector t that starts one float into its buffer (4 bytes past a 16-byte boundary)"""
    buf = torch.zeros(t.numel() + 5, dtype=torch.float32, device="cuda")
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# =============================================================================================== A. norms
class NormRef:
    """float64 LayerNorm / RMSNorm of x [rows, dim] and its gradients by autograd"""

    def __init__(self, x, g, b, kind, eps):
        self.x = x.double().requires_grad_(True)
        self.g = g.double().requires_grad_(True)
        self.b = b.double().requires_grad_(True) if b is not None else None
        mu = self.x.mean(-1, keepdim=True) if kind == 0 else torch.zeros(x.shape[0], 1, dtype=torch.float64)
        rs = torch.rsqrt(((self.x - mu) ** 2).mean(-1, keepdim=True) + eps)
        self.xhat = (self.x - mu) * rs
        self.y = self.xhat * self.g + (self.b if self.b is not None else 0.0)
        self.mu, self.rs = mu.detach()[:, 0], rs.detach()[:, 0]

    def y_as_the_kernel_rounds(self, dtype, kind):
        if dtype == BF16 and kind == 1:                  # the reference model: _norm(x.float()).type_as(x) * weight
            return q(self.xhat.detach().float(), BF16).double() * self.g.detach()
        return self.y.detach()

    def dx(self, dy):
        return torch.autograd.grad(self.y, self.x, dy.double(), retain_graph=True)[0]


def norm_eps(kind):
    return 1e-5 if kind == 0 else 1e-6


def norm_operands(rows, dim, dtype):
    x = q(rnd(rows, dim, seed=1) * 2 + 0.5, dtype)
    g, b = 1 + 0.1 * rnd(dim, seed=2), 0.1 * rnd(dim, seed=3)
    dy, dres = q(rnd(rows, dim, seed=4), dtype), q(rnd(rows, dim, seed=5), dtype)
    dyi = rint(-2, 2, rows, dim, seed=6)
    return x, g, b, dy, dres, dyi


def check_norm_fwd(K, ref, xd, gd, bd, dtype, kind, tag):
    y, mean, rstd = K.norm_fwd(xd, gd, bd, norm_eps(kind), kind)
    close(y, ref.y_as_the_kernel_rounds(dtype, kind), dtype, f"norm y {tag}")
    close(mean, ref.mu, F32, f"norm mean {tag}")
    close(rstd, ref.rs, F32, f"norm rstd {tag}")
    return y, mean, rstd


def check_norm_bwd_integer_dy(K, ref, dyi, xd, gd, mean, rstd, dtype, kind, tag):
    """integer dy without dres: dx and dgamma against float64, dbeta (a sum of small integers) bit-equal"""
    dx, dg, db = K.norm_bwd(dev(dyi, dtype), xd, gd, mean, rstd, dres=None, kind=kind, want_beta=True)
    close(dx, ref.dx(dyi), dtype, f"norm dx {tag}")
    check_colsum(dg, dyi.double() * ref.xhat.detach(), f"norm dgamma {tag}")
    assert torch.equal(db.cpu(), dyi.sum(0))
    return dx, dg, db


BF16_DIMS = [8, 72, 128, 136, 256, 264, 384, 392, 512, 520, 1000, 1024, 1032, 2048, 2056]
FP32_DIMS = [4, 68, 128, 132, 256, 260, 384, 388, 512, 516, 1000, 1024, 1028, 2048]
NORM_CASES = ([(BF16, 37, d) for d in BF16_DIMS] + [(BF16, 3, 72), (BF16, 3, 1032)] +
              [(F32, 37, d) for d in FP32_DIMS] + [(F32, 3, 68), (F32, 3, 516)])


@pytest.mark.parametrize("kind", [0, 1], ids=["layer", "rms"])
@pytest.mark.parametrize("dtype,rows,dim", NORM_CASES, ids=[f"{'bf16' if c[0] == BF16 else 'fp32'}-{c[1]}x{c[2]}" for c in NORM_CASES])
def test_norm_every_rung(K, dtype, rows, dim, kind):
    """one dim per template instantiation and one that ends inside an iteration of it; 37 rows (9 full row groups of 4 and a part of one)
    and 3 rows (less than one group)"""
    x, g, b, dy, dres, dyi = norm_operands(rows, dim, dtype)
    ref = NormRef(x, g, b if kind == 0 else None, kind, norm_eps(kind))
    xd, gd, bd = dev(x, dtype), dev(g), (dev(b) if kind == 0 else None)
    y, mean, rstd = check_norm_fwd(K, ref, xd, gd, bd, dtype, kind, "rungs")
    if kind == 1:
        assert float(mean.abs().max()) == 0.0
    dx, dg, db = K.norm_bwd(dev(dy, dtype), xd, gd, mean, rstd, dres=dev(dres, dtype), kind=kind, want_beta=(kind == 0))
    close(dx, ref.dx(dy) + dres.double(), dtype, "norm dx rungs")
    check_colsum(dg, dy.double() * ref.xhat.detach(), "norm dgamma rungs")
    if kind == 0:
        check_colsum(db, dy.double(), "norm dbeta rungs")
    else:
        assert db is None
    check_norm_bwd_integer_dy(K, ref, dyi, xd, gd, mean, rstd, dtype, kind, "rungs")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("route", ["fused", "generic"])
def test_norm_accumulate(K, dtype, route):
    """accumulate=True adds onto what dgamma / dbeta hold: the same bits as one fp32 add of the plain result, on both final kernels"""
    rows, dim = 300, 392
    x, g, b, dy, dres, dyi = norm_operands(rows, dim, dtype)
    ref = NormRef(x, g, b, 0, 1e-5)
    xd = dev(x, dtype)
    gd = misaligned(g) if route == "generic" else dev(g)
    y, mean, rstd = K.norm_fwd(xd, dev(g), dev(b), 1e-5, 0)
    dx0, dg0, db0 = K.norm_bwd(dev(dy, dtype), xd, gd, mean, rstd, dres=dev(dres, dtype))
    pre_g, pre_b = rnd(dim, seed=7) * 3, rnd(dim, seed=8) * 3
    acc_g, acc_b = dev(pre_g.clone()), dev(pre_b.clone())
    dx1, _, _ = K.norm_bwd(dev(dy, dtype), xd, gd, mean, rstd, dres=dev(dres, dtype), dgamma=acc_g, dbeta=acc_b, accumulate=True)
    assert torch.equal(dx1, dx0)
    assert torch.equal(acc_g.cpu(), pre_g + dg0.cpu()) and torch.equal(acc_b.cpu(), pre_b + db0.cpu())
    check_colsum(dg0, dy.double() * ref.xhat.detach(), f"norm dgamma {route}")
    check_colsum(db0, dy.double(), f"norm dbeta {route}")
    # integer dy onto an integer pre-fill: the accumulated dbeta is exact
    acc_b = dev(rint(-9, 9, dim, seed=9))
    K.norm_bwd(dev(dyi, dtype), xd, gd, mean, rstd, dgamma=dev(pre_g.clone()), dbeta=acc_b, accumulate=True)
    assert torch.equal(acc_b.cpu(), rint(-9, 9, dim, seed=9) + dyi.sum(0))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("route", ["fused", "generic"])
def test_norm_layer_without_dbeta(K, dtype, route):
    rows, dim = 37, 136
    x, g, b, dy, dres, _ = norm_operands(rows, dim, dtype)
    xd = dev(x, dtype)
    gd = misaligned(g) if route == "generic" else dev(g)
    y, mean, rstd = K.norm_fwd(xd, dev(g), dev(b), 1e-5, 0)
    dx0, dg0, db0 = K.norm_bwd(dev(dy, dtype), xd, gd, mean, rstd, dres=dev(dres, dtype), want_beta=True)
    dx1, dg1, db1 = K.norm_bwd(dev(dy, dtype), xd, gd, mean, rstd, dres=dev(dres, dtype), want_beta=False)
    assert db1 is None and torch.equal(dx1, dx0) and torch.equal(dg1, dg0)
    ref = NormRef(x, g, b, 0, 1e-5)
    close(dx1, ref.dx(dy) + dres.double(), dtype, f"norm dx {route}")
    check_colsum(dg1, dy.double() * ref.xhat.detach(), f"norm dgamma {route}")


@pytest.mark.parametrize("kind,which", [(0, "gamma"), (0, "beta"), (0, "both"), (1, "gamma")], ids=["layer-gamma", "layer-beta", "layer-both", "rms-gamma"])
@pytest.mark.parametrize("dim", [64, 384])
@pytest.mark.parametrize("dtype", DT)
def test_norm_misaligned_gamma_beta(K, dtype, dim, which, kind):
    """a gamma or beta that starts 4 bytes past a 16-byte boundary cannot be read as vectors: the forward (gamma or beta) and the backward
    (gamma) fall back to the generic kernels, which must give what the fast ones give"""
    rows = 37
    x, g, b, dy, dres, dyi = norm_operands(rows, dim, dtype)
    ref = NormRef(x, g, b if kind == 0 else None, kind, norm_eps(kind))
    xd = dev(x, dtype)
    gd = misaligned(g) if which in ("gamma", "both") else dev(g)
    bd = None if kind == 1 else (misaligned(b) if which in ("beta", "both") else dev(b))
    y, mean, rstd = check_norm_fwd(K, ref, xd, gd, bd, dtype, kind, "generic")
    dx, dg, db = K.norm_bwd(dev(dy, dtype), xd, gd, mean, rstd, dres=dev(dres, dtype), kind=kind, want_beta=(kind == 0))
    close(dx, ref.dx(dy) + dres.double(), dtype, "norm dx generic")
    check_colsum(dg, dy.double() * ref.xhat.detach(), "norm dgamma generic")
    if kind == 0:
        check_colsum(db, dy.double(), "norm dbeta generic")
    check_norm_bwd_integer_dy(K, ref, dyi, xd, gd, mean, rstd, dtype, kind, "generic")


WRAP_CASES = [
    # name, dtype, dim, rows, gamma misaligned
    ("fast-fwd-lpr16", F32, 64, 32768 + 37, False),          # forward: 2048 blocks x 16 rows
    ("fast-fwd-lpr16", BF16, 64, 32768 + 37, False),
    ("fast-fwd-lpr64", BF16, 1024, 8192 + 5, False),         # forward: 2048 blocks x 4 rows
    ("fused-bwd-lpr16", F32, 64, 16384 + 37, False),         # backward: 1024 blocks x 16 rows
    ("fused-bwd-lpr16", BF16, 64, 16384 + 37, False),
    ("fused-bwd-lpr64", BF16, 1024, 4096 + 5, False),        # backward: 257 blocks x 4 rows, four passes
    ("generic", F32, 16, 32768 + 3, True),                   # generic forward and dx: 8192 blocks x 4 rows
    ("generic", BF16, 16, 32768 + 3, True),
    ("nchunks-cap", F32, 16, 131072 + 130, True),            # 513 chunks of 256 rows -> 512 of 257
    ("nchunks-cap", BF16, 16, 131072 + 130, True),
]


@pytest.mark.parametrize("kind", [0, 1], ids=["layer", "rms"])
@pytest.mark.parametrize("case", WRAP_CASES, ids=[f"{c[0]}-{'bf16' if c[1] == BF16 else 'fp32'}" for c in WRAP_CASES])
def test_norm_grid_wraps(K, case, kind):
    """more rows than one pass of the capped grid covers, by a ragged remainder: every row written once, every row summed once"""
    _, dtype, dim, rows, mis = case
    x, g, b, _, _, dyi = norm_operands(rows, dim, dtype)
    ref = NormRef(x, g, b if kind == 0 else None, kind, norm_eps(kind))
    xd = dev(x, dtype)
    gd = misaligned(g) if mis else dev(g)
    bd = dev(b) if kind == 0 else None
    y, mean, rstd = check_norm_fwd(K, ref, xd, gd, bd, dtype, kind, "wraps")
    check_norm_bwd_integer_dy(K, ref, dyi, xd, gd, mean, rstd, dtype, kind, "wraps")


def test_norm_bwd_refuses_null_mean(K):
    """LayerNorm's backward reads mean[row]: a null pointer is refused before any launch; RMSNorm never reads it and takes one"""
    from frankenstein_amd import _lib
    rows, dim = 8, 64
    x, g, b, dy, _, _ = norm_operands(rows, dim, F32)
    xd, gd, dyd = dev(x), dev(g), dev(dy)

    def bwd(kind, mean, rstd):
        dx, dg, db = (torch.empty(rows, dim, device="cuda"), torch.empty(dim, device="cuda"), torch.empty(dim, device="cuda"))
        ws = torch.empty(_lib.lib().fk_norm_bwd_workspace_bytes(rows, dim), dtype=torch.uint8, device="cuda")
        _lib.call("fk_norm_bwd", dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), None if mean is None else mean.data_ptr(), rstd.data_ptr(), None,
                  dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, dim, kind, 0, _lib.FK_F32, ws.data_ptr(), ws.numel(),
                  torch.cuda.current_stream().cuda_stream)
        return dx

    _, mean, rstd = K.norm_fwd(xd, gd, dev(b), 1e-5, 0)
    with pytest.raises(_lib.FrankenHipError, match="null pointer"):
        bwd(0, None, rstd)
    bwd(0, mean, rstd)
    _, mean1, rstd1 = K.norm_fwd(xd, gd, None, 1e-6, 1)
    assert torch.equal(bwd(1, None, rstd1), bwd(1, mean1, rstd1))


# =============================================================================================== B. colsum
COLSUM_CASES = [
    # name, rows, cols, ld, base offset (elements), dtypes
    ("scalar-cols203", 300, 203, 203, 0, DT),
    ("scalar-ld201", 300, 200, 201, 0, DT),
    ("scalar-base1", 300, 200, 200, 1, DT),
    ("vector-two-chunks-fp32", 300, 1100, 1100, 0, [F32]),          # 275 vectors: 256 + 19
    ("vector-two-chunks-bf16", 300, 2120, 2120, 0, [BF16]),         # 265 vectors: 256 + 9
    ("vector-two-full-chunks-fp32", 300, 2048, 2048, 0, [F32]),     # 512 vectors: the last one of the second chunk is the row's last
    ("vector-two-full-chunks-bf16", 300, 4096, 4096, 0, [BF16]),
    ("vector-ld200", 300, 192, 200, 0, DT),
    ("vector-block-cap", 131072 + 77, 8, 8, 0, DT),                 # 513 row blocks -> 512 of 257 rows
    ("scalar-block-cap", 131072 + 77, 7, 7, 0, DT),
]


COLSUM_PARAMS = [(c, dt) for c in COLSUM_CASES for dt in c[5]]


@pytest.mark.parametrize("case,dtype", COLSUM_PARAMS, ids=[f"{c[0]}-{'bf16' if dt == BF16 else 'fp32'}" for c, dt in COLSUM_PARAMS])
def test_colsum_exact(K, case, dtype):
    """integer operands: every column sum is exact, so the result must be bit-equal, plain and accumulated onto a pre-filled out"""
    name, rows, cols, ld, off, _ = case
    vals = rint(-3, 3, rows, cols, seed=3)
    vals[:, 0] += (torch.arange(rows) % 5).float()                  # no symmetry between rows
    buf = torch.full((rows * ld + off + 8,), 100.0, dtype=dtype, device="cuda")        # anything read outside the view shows in the sum
    x = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    x.copy_(vals)
    vec = 8 if dtype == BF16 else 4
    on_vector_path = cols % vec == 0 and ld % vec == 0 and x.data_ptr() % 16 == 0
    assert on_vector_path == name.startswith("vector")
    ref = vals.double().sum(0)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(K.colsum(x).cpu(), ref.float())
    pre = rint(-50, 50, cols, seed=4)
    out = dev(pre.clone())
    K.colsum(x, out=out, accumulate=True)
    assert torch.equal(out.cpu(), pre + ref.float())


# =============================================================================================== C. losses
def ulp_close(got, want):
    """|got - want| <= 1 ulp of want (fp32)"""
    w = np.float32(want)
    return abs(np.float32(got) - w) <= np.spacing(np.abs(w))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sq", [False, True], ids=["l1", "mse"])
def test_l1_mse_forward_exact(K, dtype, weighted, sq):
    """2051 x 129 = 264 579 elements, past the 1024-block forward grid: integer pred / target / weights make both sums exact"""
    rows, row_len = 2051, 129
    p, t = rint(-2, 2, rows, row_len, seed=1), rint(-2, 2, rows, row_len, seed=2)
    w = rint(0, 3, rows, seed=3)
    w[::7] = 0.0
    d = (p - t).double()
    f = d * d if sq else d.abs()
    wsum = (f * w.double()[:, None]).sum() if weighted else f.sum()
    cnt = w.double().sum() * row_len if weighted else float(rows * row_len)
    assert float(wsum) < 2 ** 24 and float(cnt) < 2 ** 24
    loss2 = K.l1_loss_fwd(dev(p, dtype), dev(t, dtype), sq, row_weight=dev(w) if weighted else None).cpu()
    assert float(loss2[1]) == float(cnt)
    want = np.float32(float(wsum)) / np.float32(float(cnt))
    assert ulp_close(float(loss2[0]), want), (float(loss2[0]), float(want))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sq", [False, True], ids=["l1", "mse"])
def test_l1_mse_backward_past_the_cap(K, dtype, weighted, sq):
    """8200 x 129 = 1 057 800 elements, past the 4096-block backward grid, against float64 autograd of the (weighted) mean"""
    rows, row_len = 8200, 129
    p, t = q(rnd(rows, row_len, seed=1), dtype), q(rnd(rows, row_len, seed=2), dtype)
    w = torch.rand(rows, generator=torch.Generator().manual_seed(3)) * 2
    w[::7] = 0.0
    pr = p.double().requires_grad_(True)
    d = pr - t.double()
    f = d * d if sq else d.abs()
    ref = (f * w.double()[:, None]).sum() / (w.double().sum() * row_len) if weighted else f.mean()
    (0.5 * ref).backward()
    go = torch.tensor([0.5], device="cuda")
    wd = dev(w) if weighted else None
    loss2 = K.l1_loss_fwd(dev(p, dtype), dev(t, dtype), sq, row_weight=wd)
    close(loss2[0], ref, F32, "l1/mse loss", atol32=1e-5)
    got = K.l1_loss_bwd(dev(p, dtype), dev(t, dtype), go, sq, row_weight=wd, loss2=loss2 if weighted else None)
    close(got, pr.grad, dtype, "l1/mse dpred", atol32=1e-9, rtol32=1e-5, atol16=1e-7, rtol16=1e-2)


def ce_ref(lg, tg, ignore_index):
    """float64: loss, count, lse, dlogits of mean cross entropy over the rows with a target in [0, V) other than ignore_index"""
    V = lg.shape[1]
    lr = lg.double().requires_grad_(True)
    valid = (tg != ignore_index) & (tg >= 0) & (tg < V)
    lse = torch.logsumexp(lr, -1)
    picked = lr.gather(-1, torch.where(valid, tg, torch.zeros_like(tg))[:, None])[:, 0]
    loss = ((lse - picked) * valid).sum() / valid.sum()
    loss.backward()
    return loss.detach(), int(valid.sum()), lse.detach(), lr.grad, valid


CE_SCENARIOS = ["ignore7", "seven-is-valid", "outside", "one-valid"]


@pytest.mark.parametrize("scenario", CE_SCENARIOS)
@pytest.mark.parametrize("V", [300, 50257])
@pytest.mark.parametrize("dtype", DT)
def test_cross_entropy_strides_and_targets(K, dtype, V, scenario):
    """logits read from a column slice of a wider buffer (ld != V), dlogits written into one (ldd != V, surround untouched), and
    the target rules: ignore_index other than -100, targets outside [0, V) ignored (lse still written), a single valid row"""
    rows = 21
    lg = q(rnd(rows, V, seed=1) * 2, dtype)
    tg = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(2))
    tg[tg == 7] = 8
    ign = -100
    if scenario == "ignore7":
        ign = 7
        tg[[2, 9, 20]] = 7
    elif scenario == "seven-is-valid":
        tg[[2, 9, 20]] = 7
        tg[5] = -100
    elif scenario == "outside":
        tg[1], tg[8], tg[19], tg[4] = V, V + 3, -1, -100
    else:
        tg[:] = -100
        tg[11] = V - 1
    loss, cnt, lse_ref, dref, valid = ce_ref(lg, tg, ign)
    assert cnt == {"ignore7": rows - 3, "seven-is-valid": rows - 1, "outside": rows - 4, "one-valid": 1}[scenario]
    wide = torch.full((rows, V + 24), 50.0, dtype=dtype, device="cuda")       # a logit of 50 read by mistake dominates the row
    lv = wide[:, 8:8 + V]
    lv.copy_(lg)
    loss2, lse = K.ce_loss_fwd(lv, dev(tg), ignore_index=ign)
    close(loss2[0], loss, F32, "ce loss")
    assert float(loss2[1]) == cnt
    close(lse, lse_ref, F32, "ce lse")
    dbuf = torch.empty(rows, V + 40, dtype=dtype, device="cuda")
    dbuf.fill_(7.0)
    go = torch.ones(1, device="cuda")
    dl = K.ce_loss_bwd(lv, dev(tg), lse, loss2, go, dbuf[:, 16:16 + V], ignore_index=ign)
    close(dl, dref, dtype, "ce dlogits", atol32=1e-7, rtol32=1e-4, atol16=1e-3, rtol16=2e-2)
    assert float(dl[~valid.cuda()].abs().max()) == 0.0
    assert bool((dbuf[:, :16] == 7.0).all()) and bool((dbuf[:, 16 + V:] == 7.0).all())


@pytest.mark.parametrize("dtype", DT)
def test_cross_entropy_backward_past_the_cap(K, dtype):
    """84 x 50257 = 4 221 588 elements, past the 16 384-block backward grid"""
    rows, V = 84, 50257
    lg = q(rnd(rows, V, seed=1) * 2, dtype)
    tg = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(2))
    tg[3] = tg[83] = -100
    loss, cnt, lse_ref, dref, valid = ce_ref(lg, tg, -100)
    lgd = dev(lg, dtype)
    loss2, lse = K.ce_loss_fwd(lgd, dev(tg))
    close(loss2[0], loss, F32, "ce loss")
    assert float(loss2[1]) == cnt
    dl = K.ce_loss_bwd(lgd, dev(tg), lse, loss2, torch.ones(1, device="cuda"), torch.empty(rows, V, device="cuda", dtype=dtype))
    close(dl, dref, dtype, "ce dlogits", atol32=1e-7, rtol32=1e-4, atol16=1e-3, rtol16=2e-2)


@pytest.mark.parametrize("dl_dtype", DT)
def test_ce_chunked(K, dl_dtype):
    """fk_ce_chunk_fwd / _finish / _bwd over V = 300 in chunks of 128 (the last one zero-padded, 44 valid columns): the same loss, lse
    and dlogits as the whole-row float64 log-softmax; padded dlogits columns are exact zeros"""
    rows, V, cw = 21, 300, 128
    lg = rnd(rows, V, seed=1) * 2
    tg = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(2))
    tg[0], tg[1], tg[2], tg[3], tg[4], tg[5] = 5, 127, 128, 255, 256, 299          # a target in each chunk, at its edges
    tg[6] = -100
    loss, cnt, lse_ref, dref, valid = ce_ref(lg, tg, -100)
    nchunk = (V + cw - 1) // cw
    full = torch.zeros(rows, nchunk * cw, device="cuda")
    full[:, :V] = dev(lg)
    tgd = dev(tg)
    st = K.CeChunkState(rows, "cuda")
    for c in range(nchunk):
        valid_w = min(cw, V - c * cw)
        K.ce_chunk_fwd(full[:, c * cw:c * cw + valid_w], tgd, c * cw, st)
    loss2, lse = K.ce_chunk_finish(st, tgd, V)
    close(loss2[0], loss, F32, "ce chunk loss")
    assert float(loss2[1]) == cnt
    close(lse, lse_ref, F32, "ce chunk lse")
    go = torch.ones(1, device="cuda")
    parts = []
    for c in range(nchunk):
        dl = torch.empty(rows, cw, dtype=dl_dtype, device="cuda")
        K.ce_chunk_bwd(full[:, c * cw:(c + 1) * cw], tgd, c * cw, min(cw, V - c * cw), lse, loss2, go, dl, V)
        parts.append(dl)
    cat = torch.cat(parts, 1)
    close(cat[:, :V], dref, dl_dtype, "ce chunk dlogits", atol32=1e-7, rtol32=1e-4, atol16=1e-3, rtol16=2e-2)
    assert float(cat[:, V:].abs().max()) == 0.0 and not bool(torch.isnan(cat).any())
    assert float(cat[6].abs().max()) == 0.0


# =============================================================================================== D. AdamW
def adamw_check(K, n, step, lr, wd, clip, gscale, zero_grad, m0=None, v0=None):
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2) * 3
    m0 = torch.zeros(n) if m0 is None else m0
    v0 = torch.zeros(n) if v0 is None else v0
    geff = g0.double() * gscale
    if clip > 0:
        geff = RT.clip_grad_value(geff, clip)
    pr, mr, vr = RT.adamw_step(p0.double(), geff, m0.double(), v0.double(), step, lr, wd)
    pd, gd, md, vd = dev(p0.clone()), dev(g0.clone()), dev(m0.clone()), dev(v0.clone())
    K.adamw_step_(pd, gd, md, vd, step, lr, weight_decay=wd, clip=clip, grad_scale=gscale, zero_grad=zero_grad)
    for got, want, atol in ((pd, pr, 2e-7), (md, mr, 2e-7), (vd, vr, 1e-9)):
        torch.testing.assert_close(got.cpu(), want.float(), rtol=2e-6, atol=atol)
    if zero_grad:
        assert int(torch.count_nonzero(gd)) == 0
    else:
        assert torch.equal(gd.cpu(), g0)


@pytest.mark.parametrize("case", ["tail-only", "no-weight-decay", "step-1000", "tail-zero-grad"])
def test_adamw_small(K, case):
    if case == "tail-only":
        adamw_check(K, 3, 1, 1e-3, 1e-5, 0.0, 1.0, False)
    elif case == "no-weight-decay":
        adamw_check(K, 1003, 2, 1e-3, 0.0, 1.0, 1.0, False, m0=rnd(1003, seed=3) * 0.1, v0=rnd(1003, seed=4).abs() * 0.1)
    elif case == "step-1000":
        adamw_check(K, 1003, 1000, 3e-4, 1e-2, 0.0, 1.0, False, m0=rnd(1003, seed=3) * 0.1, v0=rnd(1003, seed=4).abs() * 0.1)
    else:
        adamw_check(K, 7, 3, 1e-3, 1e-5, 0.5, 0.25, True)


def test_adamw_body_wrap_and_tail(K):
    """n = 4 x 4096 x 256 + 4 x 300 + 3: 300 float4 past one pass of the 4096-block grid and a 3-element tail; zero_grad, clip and
    grad_scale together; every gradient element zeroed"""
    n = 4 * 4096 * 256 + 4 * 300 + 3
    adamw_check(K, n, 5, 1e-3, 1e-5, 0.5, 0.25, True)


# =============================================================================================== E. pointwise stride loops
def two_ranges(fn, parts, full):
    """fn over each of the row ranges `parts` (each under the cap) must give the bits of the one call over everything"""
    lo = 0
    for args in parts:
        got = fn(*args)
        assert torch.equal(got, full[lo:lo + got.shape[0]])
        lo += got.shape[0]
    assert lo == full.shape[0]


def ends(n, k=65536):
    """index ranges of the first and the last k of n"""
    return (slice(0, min(k, n)), slice(max(0, n - k), n))


@pytest.mark.parametrize("dtype", DT)
def test_swiglu_past_the_cap(K, dtype):
    vec = 8 if dtype == BF16 else 4
    H, rows = 5 * vec, WORK // 5                                   # 5 vectors per row: WORK vectors of work
    assert rows * (H // vec) == WORK
    h13, dg = drnd(rows, 2 * H, seed=1, dtype=dtype), drnd(rows, H, seed=2, dtype=dtype)
    g, d = K.swiglu_fwd(h13), K.swiglu_bwd(h13, dg)
    r0 = rows // 2
    two_ranges(K.swiglu_fwd, [(h13[:r0],), (h13[r0:],)], g)
    two_ranges(K.swiglu_bwd, [(h13[:r0], dg[:r0]), (h13[r0:], dg[r0:])], d)
    for sl in ends(rows, 65536 // H + 1):
        hr = h13[sl].double().cpu().requires_grad_(True)
        gref = hr[:, :H] * torch.sigmoid(hr[:, :H]) * hr[:, H:]
        close(g[sl], gref, dtype, "swiglu fwd", atol32=1e-6)
        gref.backward(dg[sl].double().cpu())
        close(d[sl], hr.grad, dtype, "swiglu bwd", atol32=2e-6)


@pytest.mark.parametrize("dtype", DT)
def test_gelu_past_the_cap(K, dtype):
    vec = 8 if dtype == BF16 else 4
    n = WORK * vec
    x, dy = drnd(n, seed=3, dtype=dtype) * 2, drnd(n, seed=2, dtype=dtype)
    y, dx = K.gelu_fwd(x), K.gelu_bwd(x, dy)
    h = (WORK // 2) * vec
    two_ranges(K.gelu_fwd, [(x[:h],), (x[h:],)], y)
    two_ranges(K.gelu_bwd, [(x[:h], dy[:h]), (x[h:], dy[h:])], dx)
    for sl in ends(n):
        xr = x[sl].double().cpu().requires_grad_(True)
        yref = 0.5 * xr * (1.0 + torch.erf(xr / math.sqrt(2.0)))
        close(y[sl], yref, dtype, "gelu fwd", atol32=1e-6)
        yref.backward(dy[sl].double().cpu())
        close(dx[sl], xr.grad, dtype, "gelu bwd", atol32=2e-6)


@pytest.mark.parametrize("dtype", DT)
def test_add_and_cast_past_the_cap(K, dtype):
    n = WORK
    a, b = drnd(n, seed=1, dtype=dtype), drnd(n, seed=2, dtype=dtype)
    y = K.add(a, b)
    h = n // 2
    two_ranges(K.add, [(a[:h], b[:h]), (a[h:], b[h:])], y)
    for sl in ends(n):
        close(y[sl], a[sl].double() + b[sl].double(), dtype, "add", atol32=0, atol16=2e-2)
    # cast: fp32 -> dtype and dtype -> fp32 (dtype = fp32: the copy instantiation), exact
    src = drnd(n, seed=3)
    c = K.cast(src, dtype)
    two_ranges(lambda s: K.cast(s, dtype), [(src[:h],), (src[h:],)], c)
    assert torch.equal(c, src.to(dtype))
    back = K.cast(c, F32)
    two_ranges(lambda s: K.cast(s, F32), [(c[:h],), (c[h:],)], back)
    assert torch.equal(back, c.float())


@pytest.mark.parametrize("dtype", DT)
def test_copy2d_past_the_cap(K, dtype):
    rows, cols = 4093, 1025                                        # 4 195 325 elements
    assert rows * cols > CAP
    src = drnd(rows, 1032, seed=1, dtype=dtype)[:, 3:3 + cols]
    dst = torch.empty(rows, 1040, dtype=dtype, device="cuda")
    dst.fill_(9.0)
    K.copy2d(src, dst[:, 7:7 + cols])
    assert torch.equal(dst[:, 7:7 + cols], src)
    assert bool((dst[:, :7] == 9.0).all()) and bool((dst[:, 7 + cols:] == 9.0).all())
    r0 = rows // 2
    two_ranges(lambda s: K.copy2d(s, torch.empty(s.shape[0], 1040, dtype=dtype, device="cuda")[:, 7:7 + cols]), [(src[:r0],), (src[r0:],)],
               dst[:, 7:7 + cols])


def test_add2d_past_the_cap(K):
    rows, cols = 4093, 1025
    g = torch.Generator(device="cuda").manual_seed(5)
    src = torch.randint(-4, 5, (rows, 1032), generator=g, device="cuda").float()[:, 3:3 + cols]
    base = torch.randint(-4, 5, (rows, 1040), generator=g, device="cuda").float()
    dst = base.clone()
    K.add2d_(dst[:, 7:7 + cols], src)
    want = base.clone()
    want[:, 7:7 + cols] += src
    assert torch.equal(dst, want)                                  # integers: exact, and the surround is untouched
    r0 = rows // 2
    two_ranges(lambda d, s: K.add2d_(d.clone()[:, 7:7 + cols], s), [(base[:r0], src[:r0]), (base[r0:], src[r0:])], dst[:, 7:7 + cols])


@pytest.mark.parametrize("dtype", DT)
def test_rope_past_the_cap(K, dtype):
    vec = 8 if dtype == BF16 else 4
    # D = one vector on purpose: WORK is odd, so only an odd number of vectors per row gives exactly 771 past the cap.  The offset inside
    # a head's table row (d / 2 > 0) is test_kernels_gpu.py's ground; here the table row t = row % T and the head stride past the cap are.
    D, nh, B, T = vec, 5, 5, WORK // 25                            # 5 vectors per row, B * T = WORK / 5 rows
    assert B * T * (nh * D // vec) == WORK
    ld = (nh + 1) * D                                              # one head-width of columns that must stay as they are
    ang = torch.rand(T, D // 2, generator=torch.Generator().manual_seed(1)) * 6.28
    table = dev(torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous())
    x0 = drnd(B, T, ld, seed=2, dtype=dtype)
    x = K.rope_(x0.clone(), nh, D, table)
    two_ranges(lambda t: K.rope_(t.clone(), nh, D, table), [(x0[:3],), (x0[3:],)], x)
    assert torch.equal(x[..., nh * D:], x0[..., nh * D:])
    R = 65536 // ld + 1
    tb = table.double().cpu()
    for b, ts in ((0, slice(0, R)), (B - 1, slice(T - R, T))):
        v = x0[b, ts, :nh * D].double().cpu().view(-1, nh, D // 2, 2)
        c, s = tb[ts, None, :, 0], tb[ts, None, :, 1]
        want = torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], -1).reshape(-1, nh * D)
        close(x[b, ts, :nh * D], want, dtype, "rope", atol32=1e-6, atol16=2e-2)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("W", [24, 20], ids=["vector", "scalar"])
def test_gather_rows_past_the_cap(K, dtype, W):
    """W = 24: the vector kernel (4096 blocks x 4 waves x 21 rows = 344 064 rows a pass); W = 20: the element-wise one (16 384 x 256)"""
    B, n, N = (3, 114943, 120000) if W == 24 else (3, 70001, 71000)
    assert (B * n > 4096 * 4 * 21) if W == 24 else (B * n * W > CAP)
    src = drnd(B, N, W, seed=1, dtype=dtype)
    idx = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(i))[:n] for i in range(B)])
    idxd = dev(idx)
    g = K.gather_rows(src, idxd)
    assert torch.equal(g.cpu(), src.cpu()[torch.arange(B)[:, None], idx])
    two_ranges(K.gather_rows, [(src[:2], idxd[:2]), (src[2:], idxd[2:])], g)
    table = drnd(7, W, seed=2)
    t = K.gather_rows(table, idxd, out_dtype=dtype, idx_mod=7)
    assert torch.equal(t.cpu(), table.cpu()[idx % 7].to(dtype))
    d = torch.zeros(B, N, W, device="cuda", dtype=dtype)
    K.scatter_rows_(d, idxd, g)
    ref = torch.zeros(B, N, W).index_put((torch.arange(B)[:, None], idx), g.float().cpu())
    assert torch.equal(d.float().cpu(), ref)


@pytest.mark.parametrize("dtype", DT)
def test_scatter_add_rows_past_the_cap(K, dtype):
    rows, W, Nt = 210003, 20, 1000                                 # 4 200 060 atomic adds of small integers: exact in any order
    assert rows * W > CAP
    src = torch.randint(-2, 3, (rows, W), generator=torch.Generator().manual_seed(1)).float()
    idx = torch.randint(0, 3 * Nt, (rows,), generator=torch.Generator().manual_seed(2))
    acc = torch.zeros(Nt, W, device="cuda")
    K.scatter_add_rows_(acc, dev(idx), dev(src, dtype), idx_mod=Nt)
    ref = torch.zeros(Nt, W, dtype=torch.float64).index_add_(0, idx % Nt, src.double())
    assert torch.equal(acc.cpu(), ref.float())
    two = torch.zeros(Nt, W, device="cuda")
    for sl in (slice(0, rows // 2), slice(rows // 2, rows)):
        K.scatter_add_rows_(two, dev(idx[sl]), dev(src[sl], dtype), idx_mod=Nt)
    assert torch.equal(two, acc)


@pytest.mark.parametrize("dtype", DT)
def test_gpt_embed_past_the_cap(K, dtype):
    B, tc, tw, d, V = 7, 5, 9360, 64, 211                          # 7 x 9365 x 64 = 4 195 520 elements
    assert B * (tc + tw) * d > CAP
    idx = torch.randint(0, V, (B, tw), generator=torch.Generator().manual_seed(1))
    prefix, wte, wpe = q(rnd(B, tc, d, seed=2), dtype), rnd(V, d, seed=3), rnd(tc + tw, d, seed=4)
    pd, wted, wped, idxd = dev(prefix, dtype), dev(wte), dev(wpe), dev(idx)
    out = K.gpt_embed_fwd(idxd, pd, wted, wped, dtype)
    two_ranges(lambda i, p: K.gpt_embed_fwd(i, p, wted, wped, dtype), [(idxd[:4], pd[:4]), (idxd[4:], pd[4:])], out)
    want = torch.cat([prefix.double(), wte.double()[idx]], 1) + wpe.double()
    for b, ts in ((0, slice(0, 1024)), (B - 1, slice(tc + tw - 1024, tc + tw))):
        close(out[b, ts], want[b, ts], dtype, "gpt embed", atol32=1e-6, atol16=3e-2)


@pytest.mark.parametrize("dtype", DT)
def test_dropout_past_the_cap(K, dtype):
    """keep mask and scale against the host restatement over the first and the last 65 536 elements of one call past the cap"""
    from tests import dropout_ref as DR
    vec = 8 if dtype == BF16 else 4
    n, p, seed, step, site = WORK * vec, 0.25, 1234567, 5, 3
    x = (drnd(n, seed=1).abs() + 0.5).to(dtype)                    # no zeros: a zero output is a dropped element
    res = drnd(n, seed=2, dtype=dtype)
    words = torch.tensor([seed, step], dtype=torch.int32, device="cuda")
    y, y2 = K.dropout(x, p, words, site), K.dropout(x, p, words, site, residual=res)
    ks = 1.0 / (1.0 - float(np.float32(p)))
    for sl in ends(n):
        keep = torch.from_numpy(DR.keep(seed, step, site, 0, np.arange(sl.start, sl.stop, dtype=np.uint64), p))
        assert torch.equal(y[sl].cpu() != 0, keep)
        want = torch.where(keep, x[sl].double().cpu() * ks, torch.zeros((), dtype=torch.float64))
        close(y[sl], want, dtype, "dropout", atol32=1e-6, rtol32=1e-6, atol16=0.0, rtol16=8e-3)
        assert torch.equal(y2[sl].cpu() != res[sl].cpu(), keep)
        close(y2[sl], want + res[sl].double().cpu(), dtype, "dropout + residual", atol32=1e-6, rtol32=1e-6, atol16=4e-2, rtol16=8e-3)
    h = (WORK // 2) * vec                                          # the first half alone: the same stream (the index is the element's)
    assert torch.equal(K.dropout(x[:h], p, words, site), y[:h])


# =============================================================================================== F. weight-shadow packing, add2d_
def test_add2d_strided_views(K):
    rows, cols = 37, 50
    src_buf, dst_buf = rint(-5, 5, rows, 64, seed=1), rint(-5, 5, rows, 72, seed=2)
    sd, dd = dev(src_buf), dev(dst_buf)
    K.add2d_(dd[:, 11:11 + cols], sd[:, 3:3 + cols])
    want = dst_buf.clone()
    want[:, 11:11 + cols] += src_buf[:, 3:3 + cols]
    assert torch.equal(dd.cpu(), want)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("shape", [(24, 40), (1500, 1400)], ids=["small", "past-the-cap"])
def test_cast_pack_rows(K, dtype, transpose, shape):
    """the SwiGLU interleave (rblk 4, rstride 8, roff 0 / 4) against index arithmetic; 1500 x 1400 is past the 8192-block grid"""
    H, Kd = shape
    w1, w3 = rnd(H, Kd, seed=1), rnd(H, Kd, seed=2)
    dst = torch.empty((Kd, 2 * H + 8) if transpose else (2 * H, Kd + 8), dtype=dtype, device="cuda")
    dst.fill_(5.0)
    view = dst[:, :2 * H] if transpose else dst[:, :Kd]
    K.cast_pack_rows(dev(w1), view, transpose, 4, 8, 0)
    K.cast_pack_rows(dev(w3), view, transpose, 4, 8, 4)
    j = torch.arange(H)
    want = torch.zeros(2 * H, Kd)
    want[(j // 4) * 8 + j % 4] = q(w1, dtype)
    want[(j // 4) * 8 + j % 4 + 4] = q(w3, dtype)
    got = view.float().cpu()
    assert torch.equal(got, want.t() if transpose else want)
    assert bool((dst[:, (2 * H if transpose else Kd):] == 5.0).all())


def test_shadow_refresh_past_the_grid_cap(K):
    """fk_cast_pack_multi with more chunks than its 8192-block grid: a 2899 x 2903 parameter has 8219 plain chunks and 8281 transposed
    tiles, so blocks take a second chunk (the transposed branch passes its barriers twice); two small parameters around it, so the job
    search after the wrap sees several jobs"""
    from frankenstein_amd import engine as E
    prev = E.compute_dtype()
    E.set_compute_dtype("bf16")
    try:
        g = torch.Generator().manual_seed(11)
        small_a = torch.nn.Parameter(torch.randn(24, 40, generator=g).cuda())
        big = torch.nn.Parameter(torch.randn(2899, 2903, generator=g).cuda())
        small_b = torch.nn.Parameter(torch.randn(56, 72, generator=g).cuda())
        assert (2899 * 2903 + 1023) // 1024 > 8192 and ((2899 + 31) // 32) * ((2903 + 31) // 32) > 8192
        sh = [E.shadow([small_a]), E.shadow([big]), E.shadow([small_a], transpose=True), E.shadow([big], transpose=True),
              E.shadow([small_b]), E.shadow([small_b], transpose=True)]
        with torch.no_grad():
            for p in (small_a, big, small_b):
                p.view(-1)[:] = torch.randn(p.numel(), generator=g).cuda()     # in place through a view, like the optimizer
        E.bump_weight_epoch()
        E.refresh_shadows([small_a, big, small_b])
        for plain, tr, p in ((sh[0], sh[2], small_a), (sh[1], sh[3], big), (sh[4], sh[5], small_b)):
            assert torch.equal(plain, p.detach().bfloat16()) and torch.equal(tr, p.detach().bfloat16().t())
        assert E.shadow([big]) is sh[1] and E.shadow([big], transpose=True) is sh[3]      # lookups, no re-pack
    finally:
        E.set_compute_dtype(prev)
