"""Every path of the fused vocabulary head + cross entropy (csrc/head_ce.hip) on the MI355X against float64, on the operands of
tests/head_ce_cases.py: exact small integers (every logit exact in fp32, every operand exact in bf16), strided H / W views, 1024 in every
row of W and entry of bias at and past V.  The case table, the reference, the bounds and the check functions live in
tests/head_ce_cases.py; tests/test_head_ce_cpu.py pins what each case reaches and shows that the checks reject a lost column, a lost or
doubled part, a misplaced target, leaked padding rows, a hard-coded ignore_index, an untransposed store and a lost half tile of db.

    branch or limit                                              source                                     test (case rows x V x K)
    -----------------------------------------------------------  -----------------------------------------  ---------------------------------------
    one part, `part < npart` false for wave wn = 1 (64 columns   head_ce_kernel<T, 0> epilogue              test_forward / test_backward 70x40x8
      wholly past V: maximum -inf, sum 0); rows 64..69 the only
      valid ones of wave wm = 1
    one k-tile of one 16-byte piece (bf16), of two (fp32)        gload, `k < p.K`                           70x40x8
    exact tile and part edges, nk = 1 (bf16) / 2 (fp32)          the k loop                                 128x64x64
    one row in the second row tile; 3 parts in 2 column tiles;   `m0 + row < p.rows`, `part < npart`        129x129x72
      partial last k-tile (8 of 64 / 32); nk = 2 / 3: both
      parities of the double buffer
    V % 8 != 0 (npad 216 / 212), rows % 4 != 0, nk = 3 / 5       `n < p.V`, the 4-row store of dlT          203x211x160
    66 parts: the merge loop's second pass (two lanes);          head_ce_merge_kernel `i += 64`;            66x4161x16
      33 tiles: xcd_remap with a remainder                       xcd_remap
    K = 768 (GPT-2): 12 / 24 k-tiles, 9 tiles                    the k loop                                 333x300x768
    V = 50257 (GPT-2): 786 parts, 393 tiles                      merge loop, grid                           70x50257x32
    ldh > K, ldw > K, wrows > V, rows of W past V = 1024          `n0 + row < p.wrows`, `ok = n < p.V`       every case
    bias on / off, bias entries past V = 1024                    `bias && ok`                               alternate cases
    targets 0, V - 1, 63, 64, 127, 128 (part and tile edges)     `(int64_t)n == tg`                         every case
    targets V, wrows - 1, -1: nothing, counted nowhere           `tg >= 0 && tg < p.V`, fk_ce_chunk_finish  every case
    ignore_index = 3, a valid id, several rows (203x211x160;     forward: fk_ce_chunk_finish; backward:     test_ignore_index_a_valid_id
      129x129x72 for db)                                         `tg != p.ignore`
    every row ignored: count 0, loss NaN, dlT all 0 (203x211x160), `fmaxf(p.loss2[1], 1.0f)`                  test_every_row_ignored
      dlT, dbpart and db all 0 (129x129x72, with bias)
    the running maximum across parts: a spike in the first       head_ce_merge_kernel `__expf(m - M)`        test_running_maximum
      part, at column 4095, in the last part (a bias column
      raised: one run per column, every row carries the spike)
    lddl > rows_pad, sentinel columns untouched; rows_pad 64-    `n < p.vpad && mq < p.rows_pad`            test_backward (both calls)
      aligned and rows rounded up to 4; vpad = npad and a vpad
      between V and the tile edge
    dbpart: half tiles partly and wholly past rows               `lh == 0 && n < p.vpad`                    test_backward (bias cases)
    determinism: a second call returns identical bits            fixed summation order                      test_forward, test_backward
    engine.head_cross_entropy: LayerNorm + bias + ignore_index   HeadCrossEntropy                           test_engine_head_cross_entropy
      = 3 + out-of-range targets, both compute dtypes

Bounds (tests/head_ce_cases.py, none taken from the kernel): row_m / row_t bit-equal; row_s, row_lse and the loss
max(4 e32, 8 fp32 ulps of the reference) with e32 the error of torch's fp32 result on the CPU, the same for bf16; dlT
[2^-8 |ref|, bf16] + 2e-5 (p + onehot) |gout| / nvalid; db 2e-5 sum_m |dl|.  The backward runs in isolation: from the float64 row_lse
rounded to fp32 and the reference loss2.

Largest |kernel - float64| observed on an MI355X per group, the bound in force where the error came nearest to it in brackets:

    group                      fp32                          bf16
    -------------------------  ----------------------------  ----------------------------
    row_m, row_t               bit-equal, as asserted        bit-equal, as asserted
    row_s                      1.9e-6  (7.8e-6); 2.1e-4      1.9e-6  (7.8e-6); 3.5e-4 at V = 50257 (2.0e-3)
                                 at V = 50257 (2.0e-3)
    row_lse                    8.0e-7  (3.8e-6); 1.4e-6      8.0e-7  (3.8e-6); 1.4e-6 (7.6e-6)
                                 where |lse| >= 8 (7.6e-6)
    loss                       3.5e-7  (3.8e-6); 1.3e-6      8.6e-7  (3.8e-6); 1.9e-6 (7.6e-6)
                                 (7.6e-6)
    dlT                        2.1e-14 (3.2e-13): 0.07 of    1.5e-8 (1.5e-8): 0.99 of the bound — the rounding of the output to bf16 is
                                 the bound; largest 1.4e-9     the whole error and 2^-8 |ref| is its worst case; largest 3.0e-5
    db                         2.2e-12 (8.1e-11); largest    1.7e-12 (7.9e-11); largest 7.2e-9
                                 7.2e-9
    zeros, sentinels,          exact, as asserted            exact, as asserted
      second call
    engine, fp32 mode          loss 7.4e-8 (1e-5 |loss|), dx 2.5e-9, dln_w 2.9e-9, dln_b 3.5e-9, dW 1.3e-8, db 3.2e-9 (atol 1e-5)
    engine, bf16 mode          LN(x) bit-equal to the exact h; loss 1.5e-7 (2e-3 |loss|); dx 1.8e-5 (0.25 of the tolerance), dln_w 3.3e-5
                               (0.50), dln_b 3.6e-5 (0.40), dW 7.6e-5 (0.27), db 2.3e-9 (0.00): the figures the float64 emulation of the
                               bf16 storage roundings alone gives (tests/test_head_ce_cpu.py), to three digits"""
import pytest
import torch

import frankenstein_amd as fa
from tests import head_ce_cases as C

pytestmark = pytest.mark.gpu

F32, BF16 = C.F32, C.BF16
DT = [F32, BF16]
SENTINEL = -7.0


def dtid(d):
    return "bf16" if d == BF16 else "fp32"


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def operands(c):
    """H and W as views with row stride K + 8, bias with its 8 extra entries, targets — on the GPU"""
    h, w = c.hfull.cuda()[:, :c.K], c.wfull.cuda()[:, :c.K]
    assert h.stride(0) == c.K + 8 and w.stride(0) == c.K + 8 and w.shape[0] == c.path.wrows
    return h, w, (None if c.b is None else c.b.cuda()), c.tg.cuda()


def forward(K, c, tag):
    h, w, b, tg = operands(c)
    m, s, t = K.head_ce_stats(h, w, b, tg, c.V)
    C.check_stats(c, m, s, t, tag)
    loss2, lse = K.head_ce_fwd(h, w, b, tg, c.V, c.ignore_index)
    C.check_lse_loss(c, lse, loss2, tag)
    m2, s2, t2 = K.head_ce_stats(h, w, b, tg, c.V)
    loss2b, lseb = K.head_ce_fwd(h, w, b, tg, c.V, c.ignore_index)
    assert torch.equal(m, m2) and torch.equal(s, s2) and torch.equal(t, t2) and torch.equal(lse, lseb), f"{tag}: a second call differs"
    assert torch.equal(loss2.view(torch.int32), loss2b.view(torch.int32))
    return m, s


def backward(K, c, rows_pad, vpad, tag):
    """fk_head_ce_bwd from the float64 row_lse / loss2 into a [vpad, rows_pad] view of a sentinel-filled buffer -> (dlT view, db or None)"""
    h, w, b, tg = operands(c)
    r = c.ref
    lse = r.lse.float().cuda()
    loss2 = torch.tensor([r.loss, float(r.nvalid)], dtype=torch.float32).cuda()
    gout = torch.tensor([r.gout], dtype=torch.float32).cuda()
    lddl = (rows_pad + 7) // 8 * 8 + 8
    outs = []
    for _ in range(2):
        buf = torch.zeros((vpad, lddl), dtype=c.dtype, device="cuda")
        buf.fill_(SENTINEL)
        dlT = buf[:, :rows_pad]
        dbpart = torch.empty((2 * ((c.rows + 127) // 128), vpad), dtype=torch.float32, device="cuda") if c.bias else None
        K.call("fk_head_ce_bwd", h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), w.shape[0], K._ptr(b), tg.data_ptr(), lse.data_ptr(),
               loss2.data_ptr(), gout.data_ptr(), dlT.data_ptr(), lddl, rows_pad, vpad, K._ptr(dbpart), c.rows, c.V, c.K, c.ignore_index,
               K.fk_dtype(h), K._stream())
        assert bool((buf[:, rows_pad:] == SENTINEL).all()), f"{tag}: the columns beside the dlT view were written"
        outs.append((dlT, dbpart))
    assert torch.equal(outs[0][0], outs[1][0]), f"{tag}: dlT of a second call differs"
    dlT, dbpart = outs[0]
    C.check_dlT(c, dlT, tag)
    if dbpart is not None:
        assert torch.equal(dbpart, outs[1][1]) and bool(torch.isfinite(dbpart).all()), f"{tag}: dbpart"
        assert not bool(dbpart[:, c.V:].any()), f"{tag}: dbpart columns past V must be 0"
        C.check_db(c, K.colsum(dbpart)[:c.V], tag)
    return dlT


@pytest.mark.parametrize("dtype", DT, ids=dtid)
@pytest.mark.parametrize("shape", C.CASES, ids=C.cid)
def test_forward(K, shape, dtype):
    forward(K, C.make(shape, dtype), f"{C.cid(shape)} {dtid(dtype)} fwd")


@pytest.mark.parametrize("dtype", DT, ids=dtid)
@pytest.mark.parametrize("shape", C.CASES, ids=C.cid)
def test_backward(K, shape, dtype):
    c = C.make(shape, dtype)
    tag = f"{C.cid(shape)} {dtid(dtype)} bwd"
    backward(K, c, (c.rows + 63) // 64 * 64, c.path.npad, tag)                       # as engine.HeadCrossEntropy passes them
    edge = (c.V + 127) // 128 * 128
    backward(K, c, (c.rows + 3) // 4 * 4, min(c.V + 37, edge), tag + " tight")       # rows_pad = rows up to 4, V < vpad <= the tile edge


@pytest.mark.parametrize("dtype", DT, ids=dtid)
@pytest.mark.parametrize("shape", [C.IGNORE3_CASE, C.IGNORE3_BIAS_CASE], ids=C.cid)
def test_ignore_index_a_valid_id(K, shape, dtype):
    """203 x 211 x 160, and 129 x 129 x 72 for the bias gradient (dbpart, db)"""
    c = C.make(shape, dtype, 3)
    assert int((c.tg == 3).sum()) > c.rows // 7 + 2
    tag = f"{C.cid(c.shape)} {dtid(dtype)} ignore 3"
    forward(K, c, tag)
    backward(K, c, (c.rows + 63) // 64 * 64, c.path.npad, tag)


@pytest.mark.parametrize("dtype", DT, ids=dtid)
@pytest.mark.parametrize("shape", [C.IGNORE3_CASE, C.IGNORE3_BIAS_CASE], ids=C.cid)
def test_every_row_ignored(K, shape, dtype):
    """No valid row: loss2 = {NaN, 0} (the mean over nothing, as F.cross_entropy) and the backward writes zeros — it divides by
    max(loss2[1], 1), so no NaN reaches the gradient GEMMs (include/franken_hip.h).  129 x 129 x 72 has a bias: dbpart and db are
    all zeros too (backward() -> check_db)."""
    c = C.make(shape, dtype, -100, None, True)
    assert c.bias == (shape == C.IGNORE3_BIAS_CASE)
    h, w, b, tg = operands(c)
    loss2, lse = K.head_ce_fwd(h, w, b, tg, c.V, -100)
    C.check_lse_loss(c, lse, loss2, "all ignored")
    assert float(loss2[1]) == 0.0 and bool(torch.isnan(loss2[0]))
    dlT = backward(K, c, (c.rows + 63) // 64 * 64, c.path.npad, "all ignored")
    assert not bool(dlT.any())


def test_running_maximum(K):
    """One logit raised by 32 through the bias, in the first part, at column 4095 (the last the merge loop's first pass sees) and in
    the last part (its second pass): row_m is the spike exactly and row_s lies in [1, 1 + 1e-6].  The bias belongs to a column, not to
    a row, so a spike made through it cannot be given to three rows only: the reading taken here is one run per spike column, in which
    EVERY row of the case carries the spike in that column and is checked."""
    for dtype in DT:
        for col in C.spike_columns(C.SPIKE_CASE[1]):
            c = C.make(C.SPIKE_CASE, dtype, -100, col)
            m, s = forward(K, c, f"spike at {col} {dtid(dtype)}")
            assert torch.equal(m.double().cpu(), c.ref.logits[:, col])
            assert bool((s >= 1.0).all()) and bool((s <= 1.0 + 1e-6).all())


# ----------------------------------------------------------------------------------------------- engine level
@pytest.mark.parametrize("dtype", DT, ids=dtid)
def test_engine_head_cross_entropy(K, dtype):
    """engine.head_cross_entropy with LayerNorm, bias and ignore_index = 3 against float64 autograd of
    F.cross_entropy(F.linear(F.layer_norm(x), w, b)) (tests/head_ce_cases.engine_case; the rows whose target is outside [0, V) masked out
    of the reference by hand): loss, dx, the LayerNorm gradients, dW and db at the tolerances test_head_ce_fused_kernels uses for dH / dW.

    The inputs make h = LN(x) exact in bf16 (engine_case): the reference sees the operands of the products as the compute dtype holds
    them, which is what that tolerance was written for.  In bf16 mode the kernel's LN output is compared with that exact h bit for bit."""
    from frankenstein_amd import engine as E
    e = C.engine_case(dtype)
    fa.set_compute_dtype("fp32" if dtype == F32 else "bf16")
    try:
        dev = [torch.nn.Parameter(t.cuda()) for t in (e.x.to(dtype), e.ln_w, e.ln_b, e.w, e.b)]      # activations arrive in the compute dtype
        h = K.norm_fwd(dev[0].detach(), dev[1].detach(), dev[2].detach(), C.ENGINE_EPS)[0].float().cpu()
        assert torch.equal(h, e.h) if dtype == BF16 else float((h - e.h).abs().max()) < 2e-6
        loss = E.head_cross_entropy(dev[0], dev[1], dev[2], dev[3], dev[4], e.tg.cuda(), C.ENGINE_EPS, 3)
        (loss * C.ENGINE_GOUT).backward()
    finally:
        fa.set_compute_dtype("bf16")
    err = abs(float(loss.detach()) - e.loss)
    print(f"HEADCE engine loss {dtid(dtype)}: error {err:.3e}")
    assert err < (1e-5 if dtype == F32 else 2e-3) * max(1.0, abs(e.loss))
    over = []
    for (name, want), p in zip(e.grads.items(), dev):
        got = p.grad.double().cpu()
        atol, rtol = C.engine_tolerance(want, dtype)
        frac = (got - want).abs() / (atol + rtol * want.abs())
        print(f"HEADCE engine {name} {dtid(dtype)}: largest error {float((got - want).abs().max()):.3e}, |ref|max {float(want.abs().max()):.3e}, atol {atol:.3e}, "
              f"worst {float(frac.max()):.3f} of the tolerance, {int((frac > 1).sum())} of {frac.numel()} over")
        if not bool((frac <= 1).all()):
            over.append((name, round(float(frac.max()), 3), int((frac > 1).sum())))
    assert not over, f"(gradient, worst error / tolerance, elements over): {over}"
