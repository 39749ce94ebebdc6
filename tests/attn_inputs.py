"""Attention inputs on which a lost or misplaced key is a gross error, and the float64 reference they are judged by (plain helpers, no
GPU; tests/test_attn_routes_cpu.py checks that they do their job, tests/test_attn_routes_gpu.py runs the kernels on them).

Inputs.  Every operand is a small dyadic number, exactly representable in bf16, so every q.k and dO.v sum is exact in fp32 and the
reference starts from the operand values the device holds.
  * keys: the first L * w head dimensions of key j carry its ADDRESS, L digits in base w of (j * (1 + w + w^2 + ..) + 1) mod w^L (neighbouring
    keys differ in every digit), each digit as a +-1 row of the w x w Hadamard matrix; the remaining dimensions are random +-1.
  * queries: amp * (sum of the address codes of the keys the row aims at) in the address dimensions, so in log2 units (the domain of
    the pre-scaled kernels) a key scores u = amp * w (6 at D = 64) per digit it shares with a target: L * u (24) for a target, less for
    a key that collects fewer digits from all the targets together; where targets share digits with one another their codes get
    weights below 1, in steps of 1/8, that level their scores (aim()).  The remaining dimensions hold {-1, 0, 1} * 2^-4 (cross-talk
    of a fraction of a log2 unit, and a live dK column).  Pre-scaled cases hand these numbers over as Q' directly, the others multiply
    them by a power of two near 1 / (scale log2 e).
  * a row aims at (a) the visible key at its edge: its last visible key, or under a dense or key-padding mask the visible key in front of
    its first hidden one, (b) the hidden key behind (a), a decoy that scores like (a), so that wrongly including it is a gross error,
    (c) keys that cycle through the key tiles of 64 that the row sees, with the row index, as many as it takes for the rows of a query
    tile of 64 to reach every one of them; (c) is the key of its tile that shares the fewest address digits with the others.
  * v and dO are integers in [-2, 2] with an asymmetric ramp in one column (key % 7, row % 3), as in test_gemm_routes_gpu.operands.

Reference: dense softmax in float64, fully masked rows give o = 0, lse = +inf and no gradient (oracle sdpa_zero_fully_masked);
delta = rowsum(dO * O) takes the O it is handed (the device's, which is what the backward kernels read).

Bound, on every element:   |got - ref| <= [2^-8 |ref| + 2^-8 mag, bf16 only] + 2e-5 + 2e-5 mag
with mag the float64 sum of the absolute terms of the last product (o: sum_j P |v|, dv: sum_i P |dO|, dq: scale sum_j |dS| |k|,
dk: scale sum_i |dS| |q|): 2^-8 |ref| is one bf16 ulp for the stored output, 2^-8 mag one bf16 rounding of P in front of its matrix
product and one of dS in front of its products (2^-9 each), 2e-5 the project's fp32 tolerance (test_kernels_gpu.close), absolute and
relative to mag.  lse: atol = rtol = 1e-4 for both dtypes (it is fp32 on the device and the scores are exact).

Fused inverse RoPE (attn_bwd with a rope_table; tests/test_attn_rope_cpu.py, tests/test_attn_rope_gpu.py): rope_table draws angles that
keep |cos| and |sin| above 0.38, unrotate turns dq, dk and their mags by minus the angle, and the same bound holds with mag' (the
rotation is linear with coefficients of at most 1; the kernels rotate fp32 accumulators and round once at the store).

Dropout on the probabilities (attn_fwd / attn_bwd with a dropout tuple; tests/test_attn_drop_cpu.py, tests/test_attn_drop_gpu.py):
forward and backward take keep (bool, every decision predicted by tests/dropout_ref.py) and drop_scale s = fp32(1) / (fp32(1) - fp32(p))
widened: Pd = P * keep * s, o = Pd v, dv = Pd^T dO, dP = keep * s * (dO v^T), delta = rowsum(dO * O), dS = P (dP - delta); lse is the
softmax's own.  The mags go through Pd and |dS| and the bound formula is unchanged: the forward rounds the kept entries of the
unnormalised P (2^-9 each, s / l is applied in fp32 behind the product: 2^-9 sum_kept P s |v| = 2^-9 mag_o), dK/dV rounds P s once in
front of P^T dO (2^-9 mag_dv) and dS is rounded once as before.  The inputs aim every row at three or more keys of equal score, so one
keep bit of a target is worth about s / 3 of |v| in o: a single wrong decision is a gross error, not only a wrong mask."""
import math

import numpy as np
import torch

from tests import dropout_ref as DR

LOG2E = 1.4426950408889634
BF, F32 = torch.bfloat16, torch.float32
TILE = 64

# head_dim -> (w, L, amp, gq): Hadamard width, digits, query amplitude in log2 units, power of two near 1 / (scale * log2 e)
LAYOUT = {8: (4, 2, 0.75, 2.0), 16: (4, 3, 1.5, 2.0), 32: (8, 3, 1.0, 4.0), 64: (8, 4, 0.75, 4.0), 128: (8, 4, 0.75, 8.0)}


def hadamard(w):
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < w:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def digits(j, w, L):
    """[n, L] digits of the address of keys j"""
    mult = sum(w ** l for l in range(L))
    a = (j * mult + 1) % (w ** L)
    return torch.stack([(a // w ** l) % w for l in range(L)], -1)


def codes(j, w, L):
    """[n, L * w] +-1 address codes of keys j"""
    return hadamard(w)[digits(j, w, L)].reshape(j.shape[0], L * w)


# ------------------------------------------------------------------------------------------------ masks
def visibility(case):
    """bool [Bm, Hm, Nq, Nk] (Bm in {1, B}, Hm in {1, H}), True = attend, and the extras a Mask needs (token ids, validity flags)"""
    B, H, Nq, Nk = case["B"], case["H"], case["Nq"], case["Nk"]
    m = case["mask"]
    kind = m[0]
    qi, ki = torch.arange(Nq)[:, None], torch.arange(Nk)[None, :]
    if kind == "none":
        return torch.ones(1, 1, Nq, Nk, dtype=torch.bool), {}
    if kind in ("causal", "block", "sliced"):
        if kind == "sliced":
            _, sub, c, full_q, full_k = m
            q_off, k_off = full_q - Nq, full_k - Nk
        else:
            sub, c, q_off, k_off = kind, (m[1] if kind == "block" else 0), 0, 0
        vis = (ki + k_off <= qi + q_off) if sub == "causal" else ((ki + k_off) // c <= (qi + q_off) // c)
        return vis[None, None], {"c": c, "q_off": q_off, "k_off": k_off, "sub": sub}
    if kind == "prefix":
        _, block, n_full = m
        assert Nq == Nk
        ids = torch.stack([torch.randperm(n_full, generator=torch.Generator().manual_seed(10 + i))[:Nq].sort()[0] for i in range(B)])
        vis = (ids[:, None, :] // block) <= (ids[:, :, None] // block)
        return vis[:, None], {"ids": ids, "block": block}
    if kind == "keypad":
        kv = torch.ones(B, Nk, dtype=torch.bool)
        for b in range(B):
            if b % 2 == 0:
                kv[b, Nk - (7 + 13 * b):] = False                    # padded tail
            else:
                kv[b, 20] = False                                     # holes: one in the first tile, one across a tile boundary
                kv[b, min(Nk - 2, 60):min(Nk - 1, 67)] = False
        if Nq == Nk:
            qv = kv.clone()
        else:
            qv = torch.ones(B, Nq, dtype=torch.bool)
            qv[:, 5::37] = False
        return (qv[:, None, :, None] & kv[:, None, None, :]), {"q_valid": qv, "k_valid": kv}
    if kind == "dense":
        _, bm, hm = m
        g = torch.Generator().manual_seed(77)
        vis = torch.rand(bm, hm, Nq, Nk, generator=g) < 0.7
        vis[..., 3::29, :] = False                                    # fully masked rows
        vis[..., :, Nk // 3:Nk // 3 + 5] = False                      # a hidden band of keys
        vis[..., 1::7, Nk // 2:] = False                              # rows that stop half way
        return vis, {}
    raise ValueError(kind)


def make_mask(K, case, extras, vis, device):
    """the kernels.Mask of the case (device = "cpu": enough for the route query, except that prefix tables need the GPU)"""
    kind = case["mask"][0]
    if kind == "none":
        return K.Mask()
    if kind in ("causal", "block", "sliced"):
        return K.Mask(K.MASK_CAUSAL if extras["sub"] == "causal" else K.MASK_BLOCK_CAUSAL, extras["c"], extras["q_off"], extras["k_off"])
    if kind == "prefix":
        if device == "cpu":
            return K.Mask(K.MASK_PREFIX, extras["block"])
        ids = extras["ids"].to(device)
        return K.Mask.from_token_ids(ids, ids, extras["block"])
    if kind == "keypad":
        if device == "cpu":
            return K.Mask(K.MASK_KEYPAD)
        return K.Mask.from_padding(extras["q_valid"].to(device), extras["k_valid"].to(device))
    m = K.Mask.from_dense(vis, case["Nq"], case["Nk"])
    m.limits = m.limits.to(device)
    return m


# ------------------------------------------------------------------------------------------------ inputs
def edge_keys(vis):
    """vis [.., Nk] bool -> (a, b): the visible edge of every row.  b = the first hidden key behind a visible one and a = b - 1; rows
    without such a step have a = their last visible key and b = their first hidden key.  -1 where there is none."""
    Nk = vis.shape[-1]
    ar = torch.arange(Nk)
    step = vis[..., :-1] & ~vis[..., 1:]
    b = torch.where(step, ar[1:], Nk).min(-1).values
    last = torch.where(vis, ar, -1).max(-1).values
    first_hidden = torch.where(~vis, ar, Nk).min(-1).values
    a = torch.where(b < Nk, b - 1, last)
    b = torch.where(b < Nk, b, first_hidden)
    b = torch.where((b < Nk) & (last >= 0), b, -1)
    return a, b


def _targets(vis_row_tile, rows, w, L):
    """for the rows (global indices) of one query tile with visibility vis_row_tile [n, Nk]: list of target key lists"""
    n, Nk = vis_row_tile.shape
    dig = [tuple(d) for d in digits(torch.arange(Nk), w, L).tolist()]
    visl = vis_row_tile.tolist()
    ea, eb = (t.tolist() for t in edge_keys(vis_row_tile))
    out = []
    for r in range(n):
        vis = visl[r]
        if ea[r] < 0:
            out.append([])
            continue
        t = [ea[r]] + ([eb[r]] if eb[r] >= 0 else [])                 # (a) the visible key at the edge, (b) the decoy behind it
        tiles = sorted({j // TILE for j in range(Nk) if vis[j]})
        i = rows[r]
        for s in range(-(-len(tiles) // n)):                          # (c) cycling through the visible key tiles
            tj = tiles[(r + s * n) % len(tiles)]
            cand = [tj * TILE + (5 * i + 11 * (i // TILE) + 17 * s + x) % TILE for x in range(TILE)]
            cand = [c for c in cand if c < Nk and vis[c] and c not in t]
            if cand:                                                  # the one that shares the fewest address digits with the others
                t.append(min(cand, key=lambda c: sum(dc == dx for x in t for dc, dx in zip(dig[c], dig[x]))))
        out.append(sorted(set(t)))
    return out


def aim(C, w, L):
    """the query direction for targets with the address codes C [T, L * w]: sum_t alpha_t C_t with the weights, in steps of 1/8, that
    give every target the score of a lone one (L digits) although targets share digits with one another: alpha = L (C C^T / w)^+ 1"""
    M = C @ C.t() / w
    alpha = torch.linalg.pinv(M, hermitian=True) @ torch.full((C.shape[0],), float(L), dtype=torch.float64)
    alpha = (torch.round(alpha * 8) / 8).clamp(0.125, 1.5)
    return (alpha[:, None] * C).sum(0)


def make_inputs(case):
    """-> dict with float64 CPU tensors q, k, v, do [B, N, H, D] (q: the UNSCALED query the reference differentiates against), q_dev (what
    is uploaded: Q' for pre-scaled cases, q otherwise), vis, extras, scale (the fp32 value the launch passes), dtype"""
    B, H, Nq, Nk, D = case["B"], case["H"], case["Nq"], case["Nk"], case["D"]
    dtype = BF if case["dtype"] == "bf16" else F32
    w, L, amp, gq = LAYOUT[D]
    A = w * L
    vis, extras = visibility(case)
    g = torch.Generator().manual_seed(1234 + Nq * 7 + Nk)
    k = torch.randint(0, 2, (B, Nk, H, D), generator=g).double() * 2 - 1
    k[..., :A] = codes(torch.arange(Nk), w, L)[None, :, None, :]
    qh = torch.randint(-1, 2, (B, Nq, H, D), generator=g).double() * 2.0 ** -4
    qh[..., :A] = 0
    cache = {}
    for bm in range(vis.shape[0]):
        for hm in range(vis.shape[1]):
            addr = torch.zeros(Nq, A, dtype=torch.float64)
            for r0 in range(0, Nq, TILE):
                rows = list(range(r0, min(Nq, r0 + TILE)))
                for i, t in zip(rows, _targets(vis[bm, hm, r0:r0 + TILE], rows, w, L)):
                    if t:
                        addr[i] = amp * aim(codes(torch.tensor(t), w, L), w, L)
            cache[bm, hm] = addr
    for b in range(B):
        for h in range(H):
            qh[b, :, h, :A] = cache[b if vis.shape[0] > 1 else 0, h if vis.shape[1] > 1 else 0]
    v = torch.randint(-2, 3, (B, Nk, H, D), generator=g).double()
    do = torch.randint(-2, 3, (B, Nq, H, D), generator=g).double()
    v[..., min(5, D - 1)] += (torch.arange(Nk) % 7).double()[None, :, None]
    do[..., min(2, D - 1)] += (torch.arange(Nq) % 3).double()[None, :, None]
    spike = case.get("spike", 0.0)
    if spike > 0:                       # a late key that outscores everything seen before by `spike` log2 units for one row per head
        i, j = Nq - 3, Nk - 70
        assert bool(vis[..., i, j].all())
        qh[:, i, :, A:] = 0
        qh[:, i, :, A] = spike
        k[:, :, :, A] = -1.0
        k[:, j, :, A] = 1.0
    if spike < 0:                       # head 0: a component shared by all keys puts every score `spike` log2 units down
        qh[:, :, 0, A] = spike / 8.0
        k[:, :, 0, A] = 8.0
    scale32 = float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32))
    if case.get("ps"):
        q_dev = qh
        q = qh / (scale32 * LOG2E)
    else:
        q_dev = q = qh * gq
    for t in (q_dev, k, v, do):
        assert torch.equal(t.to(BF).double(), t), "operands must be representable in bf16"
    return {"q": q, "q_dev": q_dev, "k": k, "v": v, "do": do, "vis": vis, "extras": extras, "scale": scale32, "dtype": dtype}


# ------------------------------------------------------------------------------------------------ reference
def drop_scale32(p):
    """the 1 / (1 - p) the device holds (fp32 arithmetic on the fp32 p), widened to float64"""
    return float(np.float32(1) / (np.float32(1) - np.float32(p)))


def case_keep(case, hi=None, lo=None, **over):
    """bool [B, H, Nq, Nk]: the keep decisions of a dropout case (tests/cases.py ATTN_DROP_CASES), predicted on the host
    (tests/dropout_ref.py).  hi(b, h, q) and lo(key) replace the two index words (integer arrays [B, 1, 1, 1], [1, H, 1, 1], [1, 1, Nq, 1]
    and [1, 1, 1, Nk] go in), seed = / step = / site = / p = replace the case's: the mutants of tests/test_attn_drop_cpu.py"""
    B, H, Nq, Nk = case["B"], case["H"], case["Nq"], case["Nk"]
    a = {n: over.get(n, case[n]) for n in ("seed", "step", "site", "p")}
    b, h = np.arange(B, dtype=np.int64).reshape(B, 1, 1, 1), np.arange(H, dtype=np.int64).reshape(1, H, 1, 1)
    q, key = np.arange(Nq, dtype=np.int64).reshape(1, 1, Nq, 1), np.arange(Nk, dtype=np.int64).reshape(1, 1, 1, Nk)
    row = (b * H + h) * Nq + q if hi is None else hi(b, h, q)
    col = key if lo is None else lo(key)
    keep = DR.keep(a["seed"], a["step"], a["site"], (row & 0xFFFFFFFF).astype(np.uint64), (col & 0xFFFFFFFF).astype(np.uint64), a["p"])
    return torch.from_numpy(np.broadcast_to(keep, (B, H, Nq, Nk)).copy())


def forward(q, k, v, vis, scale, keep=None, drop_scale=1.0):
    """q [.., Nq, D], k, v [.., Nk, D] float64, vis bool broadcastable to [.., Nq, Nk] -> o, lse, mag_o, P
    keep (bool, broadcastable to [.., Nq, Nk]) and drop_scale: dropout on the probabilities, o = Pd v with Pd = P * keep * drop_scale;
    lse and the returned P are the softmax's own (the statistics do not see the dropout)"""
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m) & (m < 0)
    e = torch.exp(s - m.masked_fill(dead, 0.0))
    l = e.sum(-1, keepdim=True)
    P = e / l.masked_fill(dead, 1.0)
    lse = (m + torch.log(l.masked_fill(dead, 1.0))).masked_fill(dead, float("inf")).squeeze(-1)
    Pd = P if keep is None else P * keep * drop_scale
    return Pd @ v, lse, Pd @ v.abs(), P


def backward(q, k, v, do, P, o_used, scale, keep=None, drop_scale=1.0):
    """-> dq, dk, dv and their mags; delta = rowsum(do * o_used)
    keep, drop_scale: dv = Pd^T do and dP = keep * drop_scale * (do v^T) go through the dropout, dS = P (dP - delta) with the softmax's P"""
    dP = do @ v.transpose(-1, -2)
    Pd = P
    if keep is not None:
        dP = dP * keep * drop_scale
        Pd = P * keep * drop_scale
    delta = (do * o_used).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    aS = dS.abs()
    return {"dq": scale * (dS @ k), "dk": scale * (dS.transpose(-1, -2) @ q), "dv": Pd.transpose(-1, -2) @ do,
            "mag_dq": scale * (aS @ k.abs()), "mag_dk": scale * (aS.transpose(-1, -2) @ q.abs()), "mag_dv": Pd.transpose(-1, -2) @ do.abs()}


def heads(t):
    """[B, N, H, D] -> [B, H, N, D]"""
    return t.transpose(1, 2)


def bound(ref, mag, dtype):
    return 2e-5 + 2e-5 * mag + (2.0 ** -8 * (ref.abs() + mag) if dtype == BF else 0.0)


def frac(got, ref, mag, dtype):
    """largest |got - ref| / bound and its index"""
    f = (got - ref).abs() / bound(ref, mag, dtype)
    f = torch.where(torch.isfinite(got), f, torch.full_like(f, float("inf")))
    return float(f.max()), int(f.argmax())


def bf16(t):
    return t.float().to(BF).double()


def rounding_model(q, k, v, do, vis, scale, dtype, store=True, keep=None, drop_scale=1.0):
    """The kernels' documented roundings on the CPU: bf16 operands round the unnormalised P in front of P V, the output O, the
    normalised P in front of P^T dO and dS in front of its two products, every output once more as it is stored, and delta comes from
    the rounded O; fp32 operands run the same products in fp32 arithmetic.  [B, H, N, D] layout.  -> o, lse, dq, dk, dv
    store=False: dq and dk as the accumulators hold them, before the rounding of the store (the fused inverse RoPE rotates them first)
    keep, drop_scale: dropout, rounded where the kernels round: the forward zeroes the dropped entries of the unnormalised P, rounds
    the kept ones and applies drop_scale / l in fp32 behind the product; dK/dV rounds P * drop_scale once in front of P^T dO; dS =
    P (keep * drop_scale * dP - delta) is rounded once, as without dropout"""
    st = bf16 if store else (lambda t: t)
    ks = None if keep is None else keep.double() * drop_scale
    if dtype == F32:
        o, lse, _, P = forward(q, k, v, vis, scale, keep, drop_scale)
        o32 = o.float()
        P32 = P.float()
        dP = do.float() @ v.float().transpose(-1, -2)
        Pd32 = P32
        if ks is not None:
            dP = dP * ks.float()
            Pd32 = P32 * ks.float()
        dS = P32 * (dP - (do.float() * o32).sum(-1, keepdim=True))
        return {"o": o32.double(), "lse": lse.float().double(), "dq": (scale * (dS @ k.float())).double(),
                "dk": (scale * (dS.transpose(-1, -2) @ q.float())).double(), "dv": (Pd32.transpose(-1, -2) @ do.float()).double()}
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m) & (m < 0)
    e = torch.exp(s - m.masked_fill(dead, 0.0))
    l = e.sum(-1, keepdim=True).masked_fill(dead, 1.0)
    lse = (m + torch.log(l)).masked_fill(dead, float("inf")).squeeze(-1)
    P = e / l
    dP = do @ v.transpose(-1, -2)
    if ks is None:
        o = bf16((bf16(e) @ v) / l)
        Pd = P
    else:
        inv = (torch.tensor(drop_scale, dtype=F32) / l.float()).double()      # drop_scale / l in fp32, behind the product
        o = bf16(((bf16(e) * keep) @ v) * inv)
        dP = dP * ks
        Pd = P * ks
    dS = bf16(P * (dP - (do * o).sum(-1, keepdim=True)))
    return {"o": o, "lse": lse.float().double(), "dq": st(scale * (dS @ k)), "dk": st(scale * (dS.transpose(-1, -2) @ q)),
            "dv": bf16(bf16(Pd).transpose(-1, -2) @ do)}


# ------------------------------------------------------------------------------------------------ fused inverse RoPE
# attn_bwd(..., rope_table=, rope_off=) rotates dq and dk by minus the angle of their row as it stores them (tests/test_attn_rope_cpu.py,
# tests/test_attn_rope_gpu.py; cases: tests/cases.py ATTN_ROPE_CASES).  The kernels take any table, so the angles here are not RoPE's:
# at RoPE's own angles most pairs of a short sequence have sin ~ 0, and a wrong sign or a neighbour's angle would hide in the tolerance.
ROPE_SLACK = 8                                                       # table rows drawn past the last one a case reads


def rope_table(Bt, rows, D, seed):
    """fp32 [Bt, rows, D / 2, 2] of (cos, sin) of theta = (pi / 2) m + pi / 8 + (pi / 4) u, m in {0, 1, 2, 3}, u in [0, 1), drawn
    independently for every sample, position and pair: |cos|, |sin| >= sin(pi / 8) = 0.38 everywhere, and neighbouring rows,
    neighbouring pairs and different samples have unrelated angles."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 4, (Bt, rows, D // 2), generator=g).double()
    u = torch.rand(Bt, rows, D // 2, generator=g, dtype=torch.float64)
    th = (math.pi / 2) * m + math.pi / 8 + (math.pi / 4) * u
    return torch.stack([torch.cos(th), torch.sin(th)], -1).float()


def case_table(case):
    """-> (tall, Tc): the case's table with ROPE_SLACK rows more than the Tc = rope_off + N it hands over (tall[:, :Tc]); the "strided"
    form hands that slice over as it stands, a view whose batch stride exceeds Tc * D"""
    Tc = case["rope_off"] + case["Nq"]
    Bt = 1 if case["table"] == "shared" else case["B"]
    return rope_table(Bt, Tc + ROPE_SLACK, case["D"], case["seed"]), Tc


def unrotate(x, mag, table, off):
    """x, mag [B, H, N, D] float64, table [Bt, rows, D / 2, 2] (Bt in {1, B}), row r of x at table row off + r.  For the pairs (d, d + 1):
    out0 = x0 c + x1 s, out1 = -x0 s + x1 c, and mag0' = |c| mag0 + |s| mag1, mag1' = |s| mag0 + |c| mag1.  The table's fp32 values are
    widened to float64: the numbers the device holds."""
    N = x.shape[2]
    t = table.double()[:, None, off:off + N]                          # [Bt, 1, N, D / 2, 2]
    c, s = t[..., 0], t[..., 1]
    x0, x1, m0, m1 = x[..., 0::2], x[..., 1::2], mag[..., 0::2], mag[..., 1::2]
    out = torch.stack([x0 * c + x1 * s, -x0 * s + x1 * c], -1).flatten(-2)
    omag = torch.stack([c.abs() * m0 + s.abs() * m1, s.abs() * m0 + c.abs() * m1], -1).flatten(-2)
    return out, omag


def unrotate_grads(ref, table, off):
    """the reference of attn_bwd with a rope_table: backward()'s dq and dk un-rotated (with their mags), dv as it is"""
    out = dict(ref)
    for n in ("dq", "dk"):
        out[n], out["mag_" + n] = unrotate(ref[n], ref["mag_" + n], table, off)
    return out
