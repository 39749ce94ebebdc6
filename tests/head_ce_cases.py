"""The cases tests/test_head_ce_cpu.py and tests/test_head_ce_gpu.py share for the fused vocabulary head + cross entropy (csrc/head_ce.hip):
the case table, the operand generator, the float64 reference and the check functions.  torch on the CPU only, so that the fp32
restatements (and their mutants) of the CPU test and the kernel's outputs in the GPU test pass through the same assertions.

Operands are small integers (tests/test_gemm_routes_gpu.operands): H in [-2, 2] with m % 3 added to one column, W in [-2, 2] with n % 2
added to one column and scaled by 2^-round(log2(2 sqrt(K))), bias integers / 4.  Every operand is exact in bf16 and every logit exact in
fp32, so bf16 is held to the fp32 bound, row_m / row_t are bit-equal to float64, and a logit deviation near 1 keeps a row's range near
10: every column carries weight in the log-sum-exp (make() asserts how much).  H and W are views with row stride K + 8; W has
wrows = V rounded up to the vector width + 8 rows and bias 8 extra entries, everything at and past V filled with 1024: a padding row
that leaks into a statistic or a gradient is a gross error, not an invisible zero.

Bounds come from the reference, never from the kernel:
    row_m, row_t     bit-equal.
    row_s, row_lse   |got - ref64| <= max(4 e32, 8 fp32 ulps of ref), both dtypes (the rule of tests/rescore_cases.tolerance); e32 = the
                     largest error of the same quantity computed in fp32 by torch on the CPU (logsumexp; sum exp(x - max)).
    loss             the same rule on the mean over the valid rows; the count is exact.
    dlT              |got - ref| <= [2^-8 |ref|, bf16] + 2e-5 (p + onehot) |gout| / nvalid on every element: check_bound of
                     tests/test_gemm_routes_gpu.py, the project's fp32 tolerance on the magnitude of the terms before the subtraction plus
                     one bf16 ulp for the single rounding of the output.  Rows >= V, columns >= rows, ignored rows and rows whose target
                     is outside [0, V): exactly 0.
    db               |got - ref| <= 2e-5 sum_m |dl_ref[m, n]| (fp32 sums of the unrounded values: the same for both dtypes)."""
import functools
import math
from types import SimpleNamespace

import torch

F32, BF16 = torch.float32, torch.bfloat16
BM = BN = 128                 # the tile of csrc/gemm_tile.h
PART = 64                     # vocabulary columns per (max, sum exp) pair: one wave's half of a tile
BK = {F32: 32, BF16: 64}
VEC = {F32: 4, BF16: 8}
FILL = 1024.0                 # rows of W and entries of bias at and past V
GOUT = 0.75
SPIKE = 32.0

#        rows,     V,   K
CASES = [(70, 40, 8), (128, 64, 64), (129, 129, 72), (203, 211, 160), (66, 4161, 16), (333, 300, 768), (70, 50257, 32)]
SPIKE_CASE = (66, 4161, 16)
IGNORE3_CASE = (203, 211, 160)
IGNORE3_BIAS_CASE = (129, 129, 72)           # ignore_index = 3 and the all-ignored sub-test once more where there is a bias: dbpart, db
EDGE_TARGETS = (63, 64, 127, 128)


def has_bias(shape):
    """bias on alternate cases (the running-maximum case needs one)"""
    return CASES.index(shape) % 2 == 0


def cid(shape):
    return "x".join(str(s) for s in shape)


def paths(shape, dtype):
    """what a case reaches, from the tile geometry alone (pinned by tests/test_head_ce_cpu.py)"""
    rows, V, K = shape
    npad = -(-V // VEC[dtype]) * VEC[dtype]
    tiles = -(-rows // BM) * -(-V // BN)
    return SimpleNamespace(nk=-(-K // BK[dtype]), k_tail=K % BK[dtype], pieces=min(K, BK[dtype]) // VEC[dtype], npart=-(-V // PART),
                           tiles=tiles, tiles_mod8=tiles % 8, npad=npad, pad=npad - V, wrows=npad + 8,
                           parts_in_last_tile=-(-V // PART) - 2 * (-(-V // BN) - 1),
                           edge_targets=tuple(t for t in EDGE_TARGETS if t < V))


def w_scale(K):
    return 2.0 ** -round(math.log2(2.0 * math.sqrt(K)))


def spike_columns(V):
    """the running-maximum probes: a column of the first part, the last column the merge loop's first pass sees, one of the last part"""
    return (5, 4095, V - 1)


def targets(shape, dtype, ignore_index, g):
    rows, V, _ = shape
    wrows = paths(shape, dtype).wrows
    tg = torch.randint(0, V, (rows,), generator=g)
    tg[::7] = ignore_index
    special = [0, V - 1] + [t for t in EDGE_TARGETS if t < V]
    free = [m for m in range(rows) if m % 7 != 0]
    for m, t in zip(free, special):
        tg[m] = t
    out = free[len(special):len(special) + 3]
    for m, t in zip(out, (V, wrows - 1, -1)):                      # outside [0, V): contribute nothing, counted nowhere
        tg[m] = t
    if ignore_index >= 0:                                          # a valid id as ignore_index: more rows that carry it
        for m in free[len(special) + 3:len(special) + 6]:
            tg[m] = ignore_index
    if rows > 65 and 65 % 7:
        tg[65] = V - 1                                             # a valid row of the second wave of rows (wm = 1)
    return tg


def lse_bound(e32, ref):
    """max(4 e32, 8 fp32 ulps of ref), elementwise (float64 tensors)"""
    ulp = torch.tensor(2.0, dtype=torch.float64) ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23)
    return torch.maximum(torch.full_like(ref, 4.0 * e32), 8.0 * ulp)


def reference(h, w, b, tg, V, ignore_index, gout=GOUT):
    """float64 reference from float64 operands h [rows, K], w [V, K], b [V] or None -> SimpleNamespace (see make())"""
    logits = h @ w.t()
    if b is not None:
        logits = logits + b
    assert torch.equal(logits.float().double(), logits), "a logit is not exact in fp32"
    rows = h.shape[0]
    m = logits.max(-1).values
    s = torch.exp(logits - m[:, None]).sum(-1)
    lse = m + torch.log(s)
    inside = (tg >= 0) & (tg < V)
    valid = inside & (tg != ignore_index)
    t = torch.where(inside, logits[torch.arange(rows), tg.clamp(0, V - 1)], torch.zeros((), dtype=torch.float64))
    nvalid = int(valid.sum())
    loss = float((lse - t)[valid].sum() / nvalid) if nvalid else float("nan")
    p = torch.exp(logits - lse[:, None])
    onehot = torch.zeros_like(p)
    onehot[torch.arange(rows)[inside], tg[inside]] = 1.0
    scale = gout / max(nvalid, 1)
    dl = (p - onehot) * scale * valid[:, None].double()
    mag = (p + onehot) * abs(scale)
    # the same quantities in fp32 by torch on the CPU: their error is the yardstick of the bounds
    x32 = logits.float()
    lse32 = torch.logsumexp(x32, -1)
    s32 = torch.exp(x32 - x32.max(-1, keepdim=True).values).sum(-1)
    e_lse = float((lse32.double() - lse).abs().max())
    e_s = float((s32.double() - s).abs().max())
    loss32 = float((lse32 - t.float())[valid].sum() / nvalid) if nvalid else float("nan")
    e_loss = abs(loss32 - loss) if nvalid else 0.0
    return SimpleNamespace(logits=logits, m=m, s=s, lse=lse, t=t, valid=valid, inside=inside, nvalid=nvalid, loss=loss, p=p, dl=dl, mag=mag,
                           db=dl.sum(0), dbmag=dl.abs().sum(0), e_lse=e_lse, e_s=e_s, e_loss=e_loss, gout=gout)


@functools.lru_cache(maxsize=None)
def make(shape, dtype, ignore_index=-100, spike=None, all_ignored=False):
    """-> SimpleNamespace(h [rows, K] and w [wrows, K] (views, row stride K + 8) and b [V + 8] or None in `dtype` on the CPU, tg int64
    [rows], hfull / wfull = the buffers h and w are views of, ref = reference(...), path = paths(...)).  spike = a column whose bias is raised by SPIKE.  Cached: treat as read-only."""
    rows, V, K = shape
    pt = paths(shape, dtype)
    g = torch.Generator().manual_seed(1000 + rows + V + K)
    hs = torch.randint(-2, 3, (rows, K + 8), generator=g).float()
    ws = torch.randint(-2, 3, (pt.wrows, K + 8), generator=g).float()
    hs[:, min(5, K - 1)] += (torch.arange(rows) % 3).float()
    ws[:, min(2, K - 1)] += (torch.arange(pt.wrows) % 2).float()
    ws *= w_scale(K)
    ws[V:] = FILL
    b = None
    if has_bias(shape):
        b = torch.randint(-4, 5, (V + 8,), generator=g).float() / 4.0
        b[V:] = FILL
        if spike is not None:
            b[spike] += SPIKE
    tg = targets(shape, dtype, ignore_index, g)
    if all_ignored:
        tg = torch.full_like(tg, ignore_index)
    hq, wq = hs.to(dtype), ws.to(dtype)
    bq = None if b is None else b.to(dtype)
    assert torch.equal(hq.float(), hs) and torch.equal(wq.float(), ws) and (b is None or torch.equal(bq.float(), b)), "operands not exact"
    assert torch.equal(hs.bfloat16().float(), hs) and torch.equal(ws.bfloat16().float(), ws), "operands not exact in bf16"
    h, w = hq[:, :K], wq[:, :K]
    ref = reference(h.double(), w[:V].double(), None if b is None else b[:V].double(), tg, V, ignore_index)
    return SimpleNamespace(shape=shape, rows=rows, V=V, K=K, dtype=dtype, ignore_index=ignore_index, h=h, w=w, hfull=hq, wfull=wq, b=bq, tg=tg, ref=ref, path=pt,
                           bias=b is not None)


# ---------------------------------------------------------------------------------------------------------------- checks
def _worst(tag, err, bound):
    frac = err / bound
    worst = float(frac.max())
    i = int(frac.argmax())
    print(f"HEADCE {tag}: worst error {float(err.reshape(-1)[i]):.3e} (bound {float(bound.reshape(-1)[i]):.3e}), largest error {float(err.max()):.3e}")
    return worst, i


def check_stats(c, row_m, row_s, row_t, tag=""):
    """row_m / row_t bit-equal to float64; row_s within max(4 e32, 8 ulps)"""
    r = c.ref
    row_m, row_s, row_t = row_m.double().cpu(), row_s.double().cpu(), row_t.double().cpu()
    assert torch.equal(row_m, r.m), f"{tag} row_m differs in rows {torch.nonzero(row_m != r.m).flatten().tolist()[:8]}"
    assert torch.equal(row_t, r.t), f"{tag} row_t differs in rows {torch.nonzero(row_t != r.t).flatten().tolist()[:8]}"
    bound = lse_bound(r.e_s, r.s)
    worst, i = _worst(f"{tag} row_s", (row_s - r.s).abs(), bound)
    assert worst <= 1.0, f"{tag} row_s of row {i}: {worst:.2f} x its bound: got {float(row_s[i])!r}, want {float(r.s[i])!r}"


def check_lse_loss(c, lse, loss2, tag=""):
    r = c.ref
    lse, loss2 = lse.double().cpu(), loss2.double().cpu()
    worst, i = _worst(f"{tag} row_lse", (lse - r.lse).abs(), lse_bound(r.e_lse, r.lse))
    assert worst <= 1.0, f"{tag} row_lse of row {i}: {worst:.2f} x its bound: got {float(lse[i])!r}, want {float(r.lse[i])!r}"
    assert float(loss2[1]) == float(r.nvalid), f"{tag} count {float(loss2[1])} != {r.nvalid}"
    if r.nvalid == 0:
        assert math.isnan(float(loss2[0])), f"{tag} the mean over no row must be NaN, got {float(loss2[0])}"
        return
    ref = torch.tensor([r.loss], dtype=torch.float64)
    worst, _ = _worst(f"{tag} loss", (loss2[:1] - ref).abs(), lse_bound(r.e_loss, ref))
    assert worst <= 1.0, f"{tag} loss: {worst:.2f} x its bound: got {float(loss2[0])!r}, want {r.loss!r}"


def check_dlT(c, dlT, tag=""):
    """dlT [vpad >= V, rows_pad >= rows] (any float dtype, CPU or GPU) against the float64 d-logits, every element"""
    r = c.ref
    got = dlT.double().cpu()
    vpad, rows_pad = got.shape
    assert vpad >= c.V and rows_pad >= c.rows and bool(torch.isfinite(got).all()), f"{tag} dlT {tuple(got.shape)} or not finite"
    ref = torch.zeros(vpad, rows_pad, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    ref[:c.V, :c.rows] = r.dl.t()
    mag[:c.V, :c.rows] = r.mag.t()
    zero = torch.ones(vpad, rows_pad, dtype=torch.bool)
    zero[:c.V, :c.rows] = ~r.valid[None, :]
    assert not bool(got[zero].any()), f"{tag} dlT must be exactly 0 past V, past rows and on rows without a valid target: {int((got[zero] != 0).sum())} are not"
    bound = 2e-5 * mag + (2.0 ** -8 * ref.abs() if c.dtype == BF16 else 0.0)
    live = ~zero
    if not bool(live.any()):
        return
    err = (got - ref).abs()
    frac = torch.where(live, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(frac.max())
    n, m = divmod(int(frac.argmax()), rows_pad)
    print(f"HEADCE {tag} dlT: worst {worst:.4f} of its bound at [{n}, {m}]: error {float(err[n, m]):.3e}, bound {float(bound[n, m]):.3e}; largest error {float(err[live].max()):.3e}")
    assert worst <= 1.0, (f"{tag} dlT[{n}, {m}]: {worst:.2f} x its bound: got {float(got[n, m])!r}, want {float(ref[n, m])!r}; "
                          f"{int((frac > 1).sum())} elements over")


def check_db(c, db, tag=""):
    r = c.ref
    got = db.double().cpu()
    assert got.shape == r.db.shape and bool(torch.isfinite(got).all())
    err, bound = (got - r.db).abs(), 2e-5 * r.dbmag
    if r.nvalid == 0:
        assert not bool(got.any()), f"{tag} db must be 0 when no row is valid"
        return
    worst, i = _worst(f"{tag} db", err, bound)
    assert worst <= 1.0, f"{tag} db[{i}]: {worst:.2f} x its bound: got {float(got[i])!r}, want {float(r.db[i])!r}"


# ---------------------------------------------------------------------------------------------------------------- fp32 restatement
MUTANTS = ("column_dropped", "part_dropped", "part_twice", "target_plus_one", "target_next_row", "padding_rows", "ignore_minus_100",
           "dlT_untransposed", "db_half_tile")


def restate(c, mutant=None, vpad=None, rows_pad=None):
    """The kernel's arithmetic in fp32 by torch on the CPU: per-part (max, sum exp) pairs merged in part order, log-sum-exp, loss, dlT
    (rounded to the compute dtype) and the bias gradient from 64-row half tiles -> SimpleNamespace(m, s, t, lse, loss2, dlT, db).
    `mutant` plants one of MUTANTS."""
    rows, V = c.rows, c.V
    vpad = c.path.npad if vpad is None else vpad
    rows_pad = -(-rows // 64) * 64 if rows_pad is None else rows_pad
    ncol = c.w.shape[0] if mutant == "padding_rows" else V
    x = c.h.float() @ c.w[:ncol].float().t()
    if c.b is not None:
        x = x + torch.cat([c.b.float(), torch.full((max(0, ncol - c.b.numel()),), FILL)])[:ncol]
    tg = c.tg.clone()
    if mutant == "target_next_row":
        tg = torch.roll(c.tg, -1)
    ignore = -100 if mutant == "ignore_minus_100" else c.ignore_index
    npart = -(-ncol // PART)
    pm = torch.full((rows, npart), -math.inf)
    ps = torch.zeros(rows, npart)
    for q in range(npart):
        xs = x[:, q * PART:(q + 1) * PART].clone()
        if mutant == "column_dropped" and q == (V // 2) // PART:
            xs[:, (V // 2) % PART] = -math.inf
        pm[:, q] = xs.max(-1).values
        ps[:, q] = torch.exp(xs - pm[:, q:q + 1]).sum(-1)
    drop = npart // 2
    if mutant == "part_dropped":
        pm[:, drop], ps[:, drop] = -math.inf, 0.0
    m = pm.max(-1).values
    wgt = torch.where(pm == -math.inf, torch.zeros_like(pm), torch.exp(pm - m[:, None]))
    if mutant == "part_twice":
        wgt[:, drop] *= 2.0
    s = (ps * wgt).sum(-1)
    inside = (tg >= 0) & (tg < V)
    tcol = (tg + (1 if mutant == "target_plus_one" else 0)).clamp(0, ncol - 1)
    t = torch.where(inside, x[torch.arange(rows), tcol], torch.zeros(()))
    lse = m + torch.log(s)
    valid = inside & (tg != ignore)
    cnt = valid.float().sum()
    loss2 = torch.stack([torch.where(valid, lse - t, torch.zeros(())).sum() / cnt, cnt])
    # backward from the float64 lse / loss2, as the GPU test runs it
    lse_in = c.ref.lse.float()
    nv = float(valid.sum()) if mutant == "ignore_minus_100" else float(c.ref.nvalid)
    gs = torch.tensor(c.ref.gout, dtype=torch.float32) / max(nv, 1.0)
    onehot = torch.zeros(rows, V)
    onehot[torch.arange(rows)[inside], tg[inside]] = 1.0
    dl = (torch.exp(x[:, :V] - lse_in[:, None]) - onehot) * gs * valid[:, None].float()
    dlT = torch.zeros(vpad, rows_pad)
    dlT[:V, :rows] = dl.t()
    if mutant == "dlT_untransposed":                               # the first 4 x 4 block of every 4-row group of dl stored as it is
        v4, r4 = V // 4 * 4, rows // 4 * 4
        blk = dlT[:v4, :r4].reshape(v4 // 4, 4, r4 // 4, 4)
        dlT[:v4, :r4] = blk.transpose(1, 3).reshape(v4, r4)
    halves = [dl[i:i + 64].sum(0) for i in range(0, rows, 64)]
    if mutant == "db_half_tile":
        halves[1] = torch.zeros(V)
    db = torch.stack(halves).sum(0)
    return SimpleNamespace(m=m, s=s, t=t, lse=lse, loss2=loss2, dlT=dlT.to(c.dtype), db=db)


def sensitivity(c):
    """-> (smallest over the columns c < V (per 64-column part above V = 4161) of the largest, over the valid rows, shift of the
    log-sum-exp when that column (part) is lost) / (the largest lse bound of a valid row)"""
    r = c.ref
    p = r.p[r.valid]
    if c.V > 4161:
        npart = -(-c.V // PART)
        pp = torch.zeros(p.shape[0], npart * PART, dtype=torch.float64)
        pp[:, :c.V] = p
        p = pp.view(p.shape[0], npart, PART).sum(-1)
    shift = -torch.log1p(-p.clamp_max(1.0 - 1e-16))
    return float(shift.max(0).values.min()) / float(lse_bound(r.e_lse, r.lse[r.valid]).max())


# ---------------------------------------------------------------------------------------------------------------- engine level
ENGINE_GOUT = 0.7
ENGINE_EPS = 0.0
ENGINE_W_SCALE = 1.0 / math.sqrt(IGNORE3_CASE[2])          # logits of deviation near 1, as the kernel-level cases


def engine_tolerance(want, dtype):
    """the tolerances of test_head_ce_fused_kernels (tests/test_kernels_gpu.py) for dH and dW -> (atol, rtol)"""
    return (1e-5, 1e-4) if dtype == F32 else (2e-3 * float(want.abs().max()) + 1e-6, 3e-2)


@functools.lru_cache(maxsize=None)
def engine_case(dtype):
    """engine.head_cross_entropy at 203 x 211 x 160 with LayerNorm, bias and ignore_index = 3, and float64 autograd of
    F.cross_entropy(F.linear(F.layer_norm(x), w, b)) over the valid rows: the rows whose target is 3 or outside [0, V) are masked out by
    hand.  -> SimpleNamespace(x, ln_w, ln_b, w, b, tg, valid, h, loss, grads)

    The tolerance the test uses (engine_tolerance) was written for a reference that sees the operands of the products as the compute
    dtype holds them.  w and b are rounded beforehand, as there.  The other operand, h = LN(x), is rounded inside the engine, where no
    reference can follow it — so, as for the kernel-level cases, the inputs make it exact: every row of x is 2^k times as many +1 as
    -1 (k = -1, 0, 1 by row) and eps = 0, hence mean 0, rstd = 2^-k and LN's normalised row is +-1; gain and shift are integers / 4, so
    that h = +-gain + shift is a multiple of 1/4 below 4, exact in bf16 and 2^-9 away from any rounding tie while the fp32 LayerNorm is
    within 1e-6 of it.  What remains between the engine and float64 are the bf16 roundings of dlT (as in the kernel-level test), of dh
    and of dx; engine_emulation() measures them and tests/test_head_ce_cpu.py holds them to 3/4 of the tolerance.  (With row mean 0,
    |normalised x| = 1 and eps = 0 this case would not notice a LayerNorm that skipped the mean subtraction: LayerNorm itself is covered
    by tests/test_rowwise_gpu.py; here it only has to hand the head an exact operand.)"""
    Fn = torch.nn.functional
    rows, V, d = IGNORE3_CASE
    g = torch.Generator().manual_seed(31)
    sign = torch.ones(rows, d)
    for m in range(rows):
        sign[m, torch.randperm(d, generator=g)[:d // 2]] = -1.0
    x = sign * (2.0 ** (torch.arange(rows) % 3 - 1).float())[:, None]
    ln_w = torch.randint(2, 7, (d,), generator=g).float() / 4.0
    ln_b = torch.randint(-2, 3, (d,), generator=g).float() / 4.0
    h = sign * ln_w + ln_b
    assert torch.equal(x.to(dtype).float(), x) and torch.equal(h.bfloat16().float(), h) and float(h.abs().max()) < 4.0
    w = (ENGINE_W_SCALE * torch.randn(V, d, generator=g)).to(dtype).float()
    b = torch.randn(V, generator=g).to(dtype).float()
    tg = targets(IGNORE3_CASE, dtype, 3, g)
    valid = (tg != 3) & (tg >= 0) & (tg < V)
    assert int((~valid).sum()) > rows // 7 + 5 and bool((tg >= V).any()) and bool((tg == -1).any())
    ref = [t.double().requires_grad_(True) for t in (x, ln_w, ln_b, w, b)]
    logits = Fn.linear(Fn.layer_norm(ref[0], (d,), ref[1], ref[2], ENGINE_EPS), ref[3], ref[4])
    loss = Fn.cross_entropy(logits[valid], tg[valid])
    (loss * ENGINE_GOUT).backward()
    assert float((logits.detach() - Fn.linear(h.double(), ref[3].detach(), ref[4].detach())).abs().max()) < 1e-12
    return SimpleNamespace(dtype=dtype, x=x, ln_w=ln_w, ln_b=ln_b, w=w, b=b, tg=tg, valid=valid, h=h, loss=float(loss.detach()),
                           grads=dict(zip(("dx", "dln_w", "dln_b", "dW", "db"), (t.grad for t in ref))))


def engine_emulation(e):
    """What the bf16 storage points of engine.HeadCrossEntropy alone cost: the same computation with every product in float64 and a
    rounding to bf16 where the engine stores bf16 (h = LN(x) — exact on these inputs —, dlT, dh, dx) -> {gradient: largest error / its
    tolerance}: how much of the tolerance the storage format uses up before any kernel arithmetic."""
    r = lambda t: t.float().to(BF16).double()
    rows, V, d = IGNORE3_CASE
    x, gam, w = e.x.double(), e.ln_w.double(), e.w.double()
    mu = x.mean(-1, keepdim=True)
    rstd = (((x - mu) ** 2).mean(-1, keepdim=True) + ENGINE_EPS).rsqrt()
    xhat = (x - mu) * rstd
    h = r(xhat * gam + e.ln_b.double())
    lg = h @ w.t() + e.b.double()
    p = torch.exp(lg - torch.logsumexp(lg, -1, keepdim=True))
    onehot = torch.zeros_like(p)
    onehot[torch.arange(rows)[e.valid], e.tg[e.valid]] = 1.0
    dl = (p - onehot) * (ENGINE_GOUT / int(e.valid.sum())) * e.valid[:, None]
    dlq = r(dl)
    dh = r(dlq @ w)
    gg = dh * gam
    got = {"dx": r(rstd * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))), "dln_w": (dh * xhat).sum(0),
           "dln_b": dh.sum(0), "dW": dlq.t() @ h, "db": dl.sum(0)}
    out = {}
    for name, v in got.items():
        want = e.grads[name]
        atol, rtol = engine_tolerance(want, BF16)
        out[name] = float(((v - want).abs() / (atol + rtol * want.abs())).max())
    return out
