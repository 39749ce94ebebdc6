"""Float64 restatement of the autograd Functions of frankenstein_amd/engine.py (AttnBranch, CrossAttnBranch, MlpBranch, NormLinear,
LayerNormFn, PatchEmbed, MaskedPatchEmbed, AssembleDecoder, GatherRows, ExpandQueries, Dropout): plain torch forward on the CPU, autograd
backward, built from the pieces of oracle/ref_models.py; dropout masks from tests/dropout_ref.py.

The same code is the ROUNDING MODEL of the engine: `reference(case, inp, rnd=Rounding(dtype))` rounds a tensor wherever the engine
stores one —
    value  -> compute dtype : shadowed weights and biases, the patch tokens, h, qkv (after RoPE and the query pre-scale), o, a, g, y
    grad   -> compute dtype : dy (cast arm of NormLinear), the gradient behind a dropout, do, dqkv (after the inverse RoPE), da, dg of
                              the unfused MLP chain, dh, dx
    grad   -> float32       : every parameter gradient; the partial sums of a column sum (bias, gamma / beta, space, mask token)
    value  -> float32       : the row statistics mean and rstd, an fp32 output
— each once, from the exact float64 value (the device accumulates in fp32 and in another order; tests/test_engine_paths_gpu.py holds
it to MARGIN times what this model loses).  With rnd=None nothing is rounded: that is the reference.

`defect` plants one bookkeeping mistake in the reference (tests/test_engine_paths_cpu.py shows that each moves a checked tensor by at
least twice the bound on every case it applies to).  Inputs are values the compute dtype holds exactly, so the reference and the
device start from the same numbers."""
import math

import numpy as np
import torch

from oracle import ref_models as R
from tests import dropout_ref as DR

MARGIN = 4.0
CDT = {"bf16": torch.bfloat16, "fp32": torch.float32}
LOG2E = 1.4426950408889634
DROP_SEED, DROP_STEP, DROP_SITES = 1234, 3, (5, 6)
LOST_ROW = 3                                     # the row the "colsum_row" defects drop


# ------------------------------------------------------------------------------------------------ rounding
class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, fwd, bwd):
        ctx.bwd = bwd
        return t.clone() if fwd is None else fwd(t)

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.bwd is None else ctx.bwd(g)), None, None


class Rounding:
    """dtype None: exact.  val / grad / act round the value, the gradient or both to the compute dtype; weight is a shadowed fp32
    master (value in the compute dtype, gradient in fp32); p32 a parameter the kernels read in fp32 (gradient in fp32)."""

    def __init__(self, dtype=None):
        self.dtype = dtype

    def c(self, t):
        return t.to(self.dtype).double()

    @staticmethod
    def f(t):
        return t.float().double()

    def _ap(self, t, fwd, bwd):
        return t if self.dtype is None else _Round.apply(t, fwd, bwd)

    def val(self, t):
        return self._ap(t, self.c, None)

    def grad(self, t):
        return self._ap(t, None, self.c)

    def act(self, t):
        return self._ap(t, self.c, self.c)

    def weight(self, t):
        return self._ap(t, self.c, self.f)

    def p32(self, t):
        return self._ap(t, None, self.f)

    def val32(self, t):
        return self._ap(t, self.f, None)


# ------------------------------------------------------------------------------------------------ inputs
def g0_pattern(n: int) -> torch.Tensor:
    """The known nonzero content of a gradient arena before the backward: small dyadic values (multiples of 1/2 up to 4)."""
    i = torch.arange(n, dtype=torch.int64)
    v = ((i * 37) % 17 - 8).double() * 0.5
    return torch.where(v == 0, torch.full_like(v, 0.5), v).float()


def _rep(t, dt):
    """values the compute dtype holds exactly, kept as float32"""
    return t.to(CDT[dt]).float()


def param_names(case):
    kw, fn = case.kw, case.fn
    if fn == "attn":
        names = (["ln_w"] if kw["norm"] != "none" else []) + (["ln_b"] if kw["norm"] == "ln" else []) + ["pw"]
        return names + (["pb", "qkv_b", "qkvw"] if kw["gpt"] else ["qw", "kw", "vw"])
    if fn == "cross":
        return ["ln_w", "ln_b", "qw", "kw", "vw", "pw"]
    if fn == "mlp":
        names = (["ln_w"] if kw["norm"] != "none" else []) + (["ln_b"] if kw["norm"] == "ln" else []) + ["up_w"]
        return names + (["up_b"] if kw["up_bias"] else []) + (["gate_w"] if kw["kind"] == "swiglu" else []) + ["down_w"] + (["down_b"] if kw["down_bias"] else [])
    if fn == "normlinear":
        return (["ln_w", "ln_b"] if kw["ln"] else []) + ["w"] + (["b"] if kw["bias"] else [])
    if fn == "layernorm":
        return ["w"] + (["b"] if kw["norm"] == "ln" else [])
    if fn in ("patch", "mpatch"):
        return ["emb_w", "emb_b", "space"]
    if fn == "assemble":
        return ["mask_token", "pos_table"]
    if fn == "expand":
        return ["q"]
    return []


def input_names(case):
    return {"cross": ["x", "context"], "gather": ["src"], "assemble": ["tokens"], "expand": [], "patch": [], "mpatch": []}.get(case.fn, ["x"])


def make_inputs(case):
    """name -> CPU tensor: activations (float32 holding compute-dtype values), fp32 master parameters, index tensors, "dy"."""
    kw, dt = case.kw, case.dtype
    g = torch.Generator().manual_seed(20240 + sum(map(ord, case.fn + case.name)))
    rn = lambda *s: torch.randn(*s, generator=g)
    lin = lambda o, i: rn(o, i) / math.sqrt(i)
    vec = lambda n: 0.3 * rn(n)
    inp = {}

    def norm_params(kind, d, pre=("ln_w", "ln_b")):
        if kind != "none":
            inp[pre[0]] = 1.0 + 0.3 * rn(d)
        if kind == "ln":
            inp[pre[1]] = vec(d)

    fn = case.fn
    if fn == "attn":
        B, N, H, D, d = (kw[k] for k in "BNHDd")
        HD = H * D
        inp["x"] = _rep(rn(B, N, d), dt)
        norm_params(kw["norm"], d)
        inp["pw"] = lin(d, HD)
        if kw["gpt"]:
            inp.update(pb=vec(d), qkv_b=vec(3 * HD), qkvw=lin(3 * HD, d))
        else:
            inp.update(qw=lin(HD, d), kw=lin(HD, d), vw=lin(HD, d))
        if kw["rope"]:
            ang = R.rope_angles(D, kw["cache"], 10000.0).double()
            if kw["rope"] == "per_sample":          # samples differ in their frequencies (a shift of the positions would cancel in q . k)
                ang = torch.stack([ang * (1.0 + 0.25 * b) for b in range(B)])
            inp["rope"] = torch.stack([torch.cos(ang), torch.sin(ang)], -1).float()      # [(B,) Tc, D/2, 2]
        if kw["mask"] == "keypad":
            kv = torch.ones(B, N, dtype=torch.bool)
            for b in range(B):
                kv[b, N - 5 - 9 * b:] = False
            inp["k_valid"] = kv
        inp["dy"] = _rep(rn(B, N, d), dt)
    elif fn == "cross":
        B, T, Nc, H, D, d = (kw[k] for k in ("B", "T", "Nc", "H", "D", "d"))
        HD = H * D
        inp["x"] = _rep(rn(B, T, d), dt)
        inp["context"] = _rep(rn(B, Nc, d), dt)
        norm_params("ln", d)
        inp.update(qw=lin(HD, d), kw=lin(HD, d), vw=lin(HD, d), pw=lin(d, HD))
        inp["dy"] = _rep(rn(B, T, d), dt)
    elif fn == "mlp":
        B, N, d, hid = (kw[k] for k in ("B", "N", "d", "hidden"))
        inp["x"] = _rep(rn(B, N, d), dt)
        norm_params(kw["norm"], d)
        inp["up_w"] = lin(hid, d)
        if kw["kind"] == "swiglu":
            inp["gate_w"] = lin(hid, d)
        if kw["up_bias"]:
            inp["up_b"] = vec(hid * (2 if kw["kind"] == "swiglu" else 1))
        inp["down_w"] = lin(d, hid)
        if kw["down_bias"]:
            inp["down_b"] = vec(d)
        inp["dy"] = _rep(rn(B, N, d), dt)
    elif fn == "normlinear":
        B, N, d, nout = (kw[k] for k in ("B", "N", "d", "nout"))
        inp["x"] = _rep(rn(B, N, d), dt)
        norm_params("ln" if kw["ln"] else "none", d)
        inp["w"] = lin(nout, d)
        if kw["bias"]:
            inp["b"] = vec(nout)
        inp["dy"] = rn(B, N, nout) if kw["out_fp32"] else _rep(rn(B, N, nout), dt)     # an fp32 output gets an fp32 gradient
    elif fn == "layernorm":
        B, N, d = (kw[k] for k in "BNd")
        inp["x"] = _rep(rn(B, N, d), dt)
        norm_params(kw["norm"], d, ("w", "b"))
        inp["dy"] = _rep(rn(B, N, d), dt)
    elif fn in ("patch", "mpatch"):
        B, nT, C, P, d = (kw[k] for k in ("B", "nT", "C", "P", "d"))
        inp["data"] = rn(B, nT * P, C)                           # fp32 recordings: no gradient
        inp.update(emb_w=lin(d, P), emb_b=vec(d), space=0.5 * rn(1, C, d))
        n = nT * C
        if fn == "mpatch":
            n = kw["n"]
            inp["unmasked"] = torch.stack([torch.randperm(nT * C, generator=g)[:n].sort().values for _ in range(B)])
        inp["dy"] = _rep(rn(B, n, d), dt)
    elif fn == "assemble":
        B, n, m, d = (kw[k] for k in "Bnmd")
        perm = torch.stack([torch.randperm(n + m, generator=g) for _ in range(B)])
        inp["unmasked"], inp["masked"] = perm[:, :n].sort(1).values, perm[:, n:].sort(1).values
        inp["tokens"] = _rep(rn(B, n, d), dt)
        inp.update(mask_token=0.5 * rn(d), pos_table=0.5 * rn(n + m, d))
        inp["dy"] = _rep(rn(B, n + m, d), dt)
    elif fn == "gather":
        B, N, n, d = (kw[k] for k in "BNnd")
        inp["src"] = _rep(rn(B, N, d), dt)
        inp["idx"] = torch.stack([torch.randperm(N, generator=g)[:n] for _ in range(B)])
        inp["dy"] = _rep(rn(B, n, d), dt)
    elif fn == "expand":
        inp["q"] = rn(1, kw["M"], kw["d"])
        inp["dy"] = _rep(rn(kw["B"], kw["M"], kw["d"]), dt)
    elif fn == "dropout":
        inp["x"] = _rep(rn(kw["B"], kw["N"], kw["d"]), dt)
        inp["dy"] = _rep(rn(kw["B"], kw["N"], kw["d"]), dt)
    else:
        raise KeyError(fn)
    if fn in ("attn", "cross", "mlp", "normlinear", "layernorm"):
        # one heavy row of dy, the row the column-sum defects lose: in bf16 the sum over the other rows carries their rounding noise
        # (it grows with the square root of the row count), and a lost row of ordinary size would sit inside it
        inp["dy"][0, LOST_ROW] *= 8.0
    return inp


def bool_mask(kw, inp):
    """[B or 1, 1, N, N] bool (True = attend) or None"""
    N, kind = kw["N"], kw["mask"]
    if kind == "none":
        return None
    if kind in ("block_causal", "dense"):
        return R.block_causal_mask(N, 8)[None, None]
    if kind == "causal":
        return torch.ones(N, N, dtype=torch.bool).tril()[None, None]
    if kind == "keypad":
        kv = inp["k_valid"]
        return kv[:, None, None, :].expand(-1, 1, N, -1)
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------ pieces
COLSUM_PARTS = 4


def _lose_row(r, v, rows, on):
    """The parameter vector v [n] as the engine's column sum sees it, broadcast to [rows, n].  The kernels add a column up in fp32 partial
    sums kept in LDS and in a workspace: the rounding model keeps COLSUM_PARTS interleaved partial sums in fp32 before the last add.
    With `on`, row LOST_ROW takes no part in the gradient (one row lost from the column sum)."""
    n = v.shape[-1]
    parts = torch.stack([r.p32(v.reshape(n)) for _ in range(COLSUM_PARTS)])
    m = parts[torch.arange(rows) % COLSUM_PARTS]
    if not on:
        return m
    return torch.cat([m[:LOST_ROW], m[LOST_ROW:LOST_ROW + 1].detach(), m[LOST_ROW + 1:]])


def _fwd_only(fx, x):
    """value fx, gradient of the identity on x"""
    return fx.detach() + x - x.detach()


def _rope(t, tab, off):
    """t [B, N, H, D], tab (cos, sin) [(B,) Tc, D/2, 2]; rows off .. off + N.  oracle.ref_models.apply_rope with the table's own fp32
    cos / sin (the numbers the kernels read) in place of the angles."""
    N = t.shape[1]
    cs = tab[off:off + N] if tab.dim() == 3 else tab[:, off:off + N]
    cs = cs.unsqueeze(-3)                                                  # [..., N, 1, D/2, 2]
    c, s = cs[..., 0], cs[..., 1]
    tp = t.reshape(*t.shape[:-1], -1, 2)
    re, im = tp[..., 0], tp[..., 1]
    return torch.stack((re * c - im * s, re * s + im * c), dim=-1).flatten(3)


def _norm(r, x, kind, w, b):
    """oracle.ref_models.layer_norm / rms_norm (the latter computes in float32, the model's x.float(): kept in float64 here) with the row
    statistics the kernels store in fp32 — mean and rstd, saved for the backward — as storage points of the rounding model, and the
    normalisation itself evaluated in fp32 (where x and dy are exact inputs, as in LayerNormFn, that arithmetic is all the error of
    dgamma there is)"""
    if kind == "ln":
        mu = r.val32(x.mean(-1, keepdim=True))
        rstd = r.val32(torch.rsqrt(((x - x.mean(-1, keepdim=True)) ** 2).mean(-1, keepdim=True) + 1e-5))
        y = r.val32(r.val32(r.val32(x - mu) * rstd) * w)           # fp32 arithmetic, one rounding per operation
        return r.val32(y + b) if b is not None else y
    return r.val32(r.val32(x * r.val32(torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6))) * w)


NORM_EPS = {"ln": 1e-5, "rms": 1e-6, "none": 0.0}


def _prenorm(x2, kind, P, r, defect):
    """h of a pre-norm branch ([rows, d]) with its storage points: h and dh; without a norm dh is stored all the same"""
    if kind == "none":
        return r.grad(x2)
    rows = x2.shape[0]
    w = _lose_row(r, r.p32(P["ln_w"]), rows, defect == ("colsum_row", "ln_w"))
    b = _lose_row(r, r.p32(P["ln_b"]), rows, defect == ("colsum_row", "ln_b")) if kind == "ln" else None
    return r.act(_norm(r, x2, kind, w, b))


def _bias(P, name, rows, r, defect):
    return _lose_row(r, r.weight(P[name]), rows, defect == ("colsum_row", name))


def _keep_scaled(keep, p):
    return torch.from_numpy(np.asarray(keep)).double() * (1.0 / (1.0 - float(np.float32(p))))


# ------------------------------------------------------------------------------------------------ the Functions
def _attn(kw, T, P, r, defect):
    B, N, H, D, d = (kw[k] for k in "BNHDd")
    M, HD = B * N, H * D
    x = r.grad(T["x"])                                                           # dx is stored once, after the residual add
    x2 = x.view(M, d)
    h = _prenorm(x2, kw["norm"], P, r, defect)
    ws = [P["qkvw"]] if kw["gpt"] else [P["qw"], P["kw"], P["vw"]]
    qkv = h @ torch.cat([r.weight(w) for w in ws]).t()
    if kw["gpt"]:
        qkv = qkv + _bias(P, "qkv_b", M, r, defect)
    prescale = kw["_proj"] in ("rope_ps", "ident_ps")
    c = (1.0 / math.sqrt(D)) * LOG2E
    q, k, v = (qkv[:, i * HD:(i + 1) * HD].view(B, N, H, D) for i in range(3))
    if defect == "dq_prescale":
        q = _fwd_only(q, q * c)
    q, k, v = r.grad(q), r.grad(k), r.grad(v)                                    # dqkv as stored: after the inverse RoPE
    if kw["rope"]:
        tab = T["rope"]
        off = tab.shape[-3] - N
        if defect == "rope_other_sample":
            tab = tab.roll(1, 0)
        rq, rk = _rope(q, tab, off), _rope(k, tab, off)
        if defect == "no_inverse_rope":
            rq, rk = _fwd_only(rq, q), _fwd_only(rk, k)
        if defect == "rope_offset":               # the backward's offset (a rotation of q AND k by one more row leaves q . k unchanged:
            bq, bk = _rope(q, tab, off - 1), _rope(k, tab, off - 1)      # the forward's offset alone is not observable)
            rq, rk = bq + (rq - bq).detach(), bk + (rk - bk).detach()
        q, k = rq, rk
    q = r.val(q * c) / c if prescale else r.val(q)
    k, v = r.val(k), r.val(v)
    mask = bool_mask(kw, T)
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))
    p = kw["drop"]
    if p:
        site = DROP_SITES[0] + (1 if defect == "attn_dropout_site" else 0)
        ks = _keep_scaled(DR.keep_attention(DROP_SEED, DROP_STEP, site, B, H, N, N, p), p)
        o = R.sdpa_dropout(qt, kt, vt, mask, ks)
    else:
        o = R.sdpa(qt, kt, vt, mask)
    o = r.act(o.transpose(1, 2).reshape(M, HD))                                  # o and do
    y = o @ r.weight(P["pw"]).t()
    if kw["gpt"]:
        y = y + _bias(P, "pb", M, r, defect)
    res = (x2.detach() if defect == "dx_residual" else x2) if kw["residual"] else 0.0
    if p:
        y = r.act(y)                                                             # y before the dropout; behind it, the dropped dy
        ks = _keep_scaled(DR.keep_flat(DROP_SEED, DROP_STEP, DROP_SITES[1], M * d, p), p).view(M, d)
        y = _fwd_only(y * ks, y) if defect == "resid_dropout_bwd" else y * ks
    return r.val(y + res).view(B, N, d)


def _cross(kw, T, P, r, defect):
    B, Tq, Nc, H, D, d = (kw[k] for k in ("B", "T", "Nc", "H", "D", "d"))
    HD = H * D
    x = r.grad(T["x"])
    x2 = x.view(B * Tq, d)
    c2 = r.grad(T["context"]).view(B * Nc, d)                                    # dctx
    h = _prenorm(x2, "ln", P, r, defect)
    q = r.act(h @ r.weight(P["qw"]).t())                                         # q, dq
    kv = r.act(c2 @ torch.cat([r.weight(P["kw"]), r.weight(P["vw"])]).t())       # kv, dkv
    qt = q.view(B, Tq, H, D).transpose(1, 2)
    kt = kv[:, :HD].view(B, Nc, H, D).transpose(1, 2)
    vt = kv[:, HD:].view(B, Nc, H, D).transpose(1, 2)
    o = r.act(R.sdpa(qt, kt, vt, None).transpose(1, 2).reshape(B * Tq, HD))
    y = o @ r.weight(P["pw"]).t() + (x2.detach() if defect == "dx_residual" else x2)
    return r.val(y).view(B, Tq, d)


def _mlp(kw, T, P, r, defect):
    B, N, d, hid = (kw[k] for k in ("B", "N", "d", "hidden"))
    M = B * N
    x = r.grad(T["x"])
    x2 = x.view(M, d)
    h = _prenorm(x2, kw["norm"], P, r, defect)
    fused = kw["_mlp"] == "swiglu_fused"
    if kw["kind"] == "swiglu":
        a = h @ torch.cat([r.weight(P["up_w"]), r.weight(P["gate_w"])]).t()
        if kw["up_bias"]:
            a = a + _bias(P, "up_b", M, r, defect)
        a = r.act(a)                                                             # a and da
        g = R.silu(a[:, :hid]) * a[:, hid:]
    else:
        a = h @ r.weight(P["up_w"]).t()
        if kw["up_bias"]:
            a = a + _bias(P, "up_b", M, r, defect)
        a = r.act(a)
        g = R.gelu_erf(a)
    g = r.val(g) if fused else r.act(g)                                          # the unfused chain stores dg; the fused ones never do
    y = g @ r.weight(P["down_w"]).t()
    if kw["down_bias"]:
        y = y + _bias(P, "down_b", M, r, defect)
    res = (x2.detach() if defect == "dx_residual" else x2) if kw["residual"] else 0.0
    p = kw["drop"]
    if p:
        y = r.act(y)
        ks = _keep_scaled(DR.keep_flat(DROP_SEED, DROP_STEP, DROP_SITES[0], M * d, p), p).view(M, d)
        y = _fwd_only(y * ks, y) if defect == "resid_dropout_bwd" else y * ks
    return r.val(y + res).view(B, N, d)


def dy_vec(dtype):
    return 8 if dtype == "bf16" else 4


def _normlinear(kw, T, P, r, defect):
    B, N, d, nout = (kw[k] for k in ("B", "N", "d", "nout"))
    M = B * N
    x2 = r.grad(T["x"]).view(M, d)
    h = _prenorm(x2, "ln" if kw["ln"] else "none", P, r, defect)
    w = r.weight(P["w"])
    y = h @ w.t()
    if defect == "dy_tail":                        # the last nout % vec columns of dy reach neither dh nor dw
        full = nout // kw["_vec"] * kw["_vec"]
        y = torch.cat([y[:, :full], y[:, full:].detach()], 1)
    if kw["bias"]:
        y = y + _bias(P, "b", M, r, defect)
    y = r.grad(y)                                  # dy in the compute dtype (a cast when the output is fp32)
    return (r.val32(y) if kw["out_fp32"] else r.val(y)).view(B, N, nout)


def _layernorm(kw, T, P, r, defect):
    B, N, d = (kw[k] for k in "BNd")
    x2 = r.grad(T["x"]).view(B * N, d)
    rows = x2.shape[0]
    w = _lose_row(r, r.p32(P["w"]), rows, defect == ("colsum_row", "w"))
    b = _lose_row(r, r.p32(P["b"]), rows, defect == ("colsum_row", "b")) if kw["norm"] == "ln" else None
    return r.val(_norm(r, x2, kw["norm"], w, b)).view(B, N, d)


def _space_rows(P, r, idx_c, defect):
    """space[0, c] per token row [rows, d]"""
    sw = r.weight(P["space"])[0]
    parts = torch.stack([r.p32(sw) for _ in range(COLSUM_PARTS)])                # fp32 partial sums, as in _lose_row
    sp = parts[torch.arange(idx_c.numel()) % COLSUM_PARTS, idx_c]
    if defect == ("colsum_row", "space"):
        sp = torch.cat([sp[:LOST_ROW], sp[LOST_ROW:LOST_ROW + 1].detach(), sp[LOST_ROW + 1:]])
    return sp


def _patch(kw, T, P, r, defect):
    B, nT, C, Pp, d = (kw[k] for k in ("B", "nT", "C", "P", "d"))
    tok = r.val(R.to_patches(T["data"], Pp)).reshape(B * nT * C, Pp)             # the patch tokens in the compute dtype
    rows = tok.shape[0]
    idx_c = torch.arange(rows) % C
    y = tok @ r.weight(P["emb_w"]).t() + _bias(P, "emb_b", rows, r, defect) + _space_rows(P, r, idx_c, defect)
    return r.val(y).view(B, nT * C, d)


def _mpatch(kw, T, P, r, defect):
    B, nT, C, Pp, d, n = (kw[k] for k in ("B", "nT", "C", "P", "d", "n"))
    tok = r.val(R.to_patches(T["data"], Pp))                                     # [B, nT * C, P]
    um = T["unmasked"]
    tok_u = torch.gather(tok, 1, um[..., None].expand(-1, -1, Pp)).reshape(B * n, Pp)
    y = tok_u @ r.weight(P["emb_w"]).t() + _bias(P, "emb_b", B * n, r, defect) + _space_rows(P, r, (um % C).reshape(-1), defect)
    return r.val(y).view(B, n, d)


def _assemble(kw, T, P, r, defect):
    B, n, m, d = (kw[k] for k in "Bnmd")
    N = n + m
    tokens = T["tokens"]
    um, mk = T["unmasked"], T["masked"]
    row = _lose_row(r, r.weight(P["mask_token"]), B * m, defect == ("colsum_row", "mask_token")).view(B, m, d)
    dec = torch.zeros(B, N, d, dtype=torch.float64)
    dec = dec.scatter(1, um[..., None].expand(-1, -1, d), tokens).scatter(1, mk[..., None].expand(-1, -1, d), row)
    order = torch.arange(N).expand(B, N) if defect == "pos_token_order" else torch.cat([um, mk], 1)
    pos = r.val(r.p32(P["pos_table"])[order])                                    # concatenation order: the reference's quirk
    return r.val(dec + pos)


def _gather(kw, T, P, r, defect):
    return torch.gather(T["src"], 1, T["idx"][..., None].expand(-1, -1, kw["d"]))


def _expand(kw, T, P, r, defect):
    return r.weight(P["q"]).expand(kw["B"], -1, -1)


def _dropout(kw, T, P, r, defect):
    p = kw["drop"]
    x = r.grad(T["x"])
    ks = _keep_scaled(DR.keep_flat(DROP_SEED, DROP_STEP, DROP_SITES[0], x.numel(), p), p).view(x.shape)
    return r.val(x * ks)


_FNS = {"attn": _attn, "cross": _cross, "mlp": _mlp, "normlinear": _normlinear, "layernorm": _layernorm, "patch": _patch,
        "mpatch": _mpatch, "assemble": _assemble, "gather": _gather, "expand": _expand, "dropout": _dropout}


def reference(case, inp, rnd=None, defect=None):
    """name -> float64 tensor: "y", "d<input>" for every differentiable input, "d<param>" for every parameter."""
    r = rnd if rnd is not None else Rounding(None)
    kw = dict(case.kw, _proj=case.paths.get("proj"), _mlp=case.paths.get("mlp"), _vec=dy_vec(case.dtype))
    P = {n: inp[n].double().requires_grad_(True) for n in param_names(case)}
    T = {n: v.double() if v.is_floating_point() else v for n, v in inp.items() if n not in P}
    ins = input_names(case)
    for n in ins:
        T[n] = T[n].requires_grad_(True)
    y = _FNS[case.fn](kw, T, P, r, defect)
    leaves = [T[n] for n in ins] + list(P.values())
    grads = torch.autograd.grad(y, leaves, T["dy"], allow_unused=True)
    out = {"y": y.detach()}
    for n, t, g in zip(ins + list(P), leaves, grads):
        out["d" + n] = torch.zeros_like(t) if g is None else g
    if defect == "up_gate_swap":
        out["dup_w"], out["dgate_w"] = out["dgate_w"], out["dup_w"]
    if defect == "qkv_split":                      # the rows of the concatenated gradient handed out one row late
        cat = torch.cat([out["dqw"], out["dkw"], out["dvw"]]).roll(1, 0)
        out["dqw"], out["dkw"], out["dvw"] = cat.split(out["dqw"].shape[0])
    return out


# ------------------------------------------------------------------------------------------------ arena
def arena_params(case):
    """the parameters whose gradient the engine accumulates itself (returns None for): the arena members of the groups and norms
    that take an in-place path"""
    if case.arena is None:
        return []
    groups = WGRAD_GROUPS[case.fn]
    names = [n for g, path in case.paths["wgrad"].items() if path != "tensors" for n in groups[g]]
    if case.paths.get("norm_bwd") == "arena":
        names += [n for n in ("ln_w", "ln_b") if n in case.arena]
    return names


def arena_layout(case, inp):
    """name -> (offset, numel) in the flat buffer, total"""
    off, lay = 0, {}
    for n in case.arena:
        lay[n] = (off, inp[n].numel())
        off += inp[n].numel()
    return lay, off


# ------------------------------------------------------------------------------------------------ bounds
U32 = 2.0 ** -24                                   # unit roundoff of float32


def bound(dtype, ref, model, kept_fp32=False):
    """per-element bound of one tensor: fp32 mode, the project's gradient bound |got - ref| <= 1e-3 |ref| + 2e-5; bf16 mode, MARGIN
    times the largest error of the rounding model relative to den = |ref| + rms(ref), times den.  For a tensor the engine keeps in fp32
    (a parameter gradient) that relative error counts as at least one unit roundoff of fp32: a sum of a few bf16 values can be exact
    in the model's order of adding and inexact in the kernel's, and MARGIN times zero allows no rounding at all."""
    ref = ref.double()
    if dtype == "fp32":
        return 1e-3 * ref.abs() + 2e-5
    den = ref.abs() + ref.pow(2).mean().sqrt()
    err = (model.double() - ref).abs()
    k = float((err / den.clamp_min(1e-300)).max()) if float(den.max()) > 0 else 0.0
    if kept_fp32:
        k = max(k, U32)
    return MARGIN * k * den


def bounds(case, ref, model):
    kept = {"d" + n for n in param_names(case)}
    return {n: bound(case.dtype, ref[n], model[n], n in kept) for n in ref}


_CACHE = {}


def case_data(case):
    """(inputs, reference, rounding model, bounds), computed once (the side-stream twin of an arena case shares them)"""
    key = (case.fn, case.name, case.dtype)
    if key not in _CACHE:
        inp = make_inputs(case)
        ref = reference(case, inp)
        model = reference(case, inp, Rounding(CDT[case.dtype]))
        _CACHE[key] = (inp, ref, model, bounds(case, ref, model))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ what the engine says it will run
WGRAD_GROUPS = {"attn": {"pw": ["pw"], "qkv": ["qw", "kw", "vw"]}, "cross": {"pw": ["pw"], "qw": ["qw"], "kv": ["kw", "vw"]},
                "mlp": {"down": ["down_w"], "up": ["up_w", "gate_w"]}}


def query_paths(case):
    """The answers of the engine's own host-side path queries for this case, in the layout of Case.paths (no GPU needed)."""
    import os
    from frankenstein_amd import engine as E, kernels as K
    kw, fn, dt = case.kw, case.fn, CDT[case.dtype]
    kinds = {"none": K.MASK_NONE, "block_causal": K.MASK_BLOCK_CAUSAL, "dense": K.MASK_DENSE, "causal": K.MASK_CAUSAL, "keypad": K.MASK_KEYPAD}
    prev, saved = E.compute_dtype(), {k: os.environ.get(k) for k in case.env}
    E.set_compute_dtype(dt)
    os.environ.update(case.env)
    try:
        out = {}
        arena = case.arena or ()
        lay = arena_layout(case, make_inputs(case))[0] if arena else {}
        names = param_names(case)
        if fn == "attn":
            out["proj"] = E.attn_proj_path(kw["B"], kw["N"], kw["H"], kw["D"], bool(kw["rope"]), kinds[kw["mask"]], bool(kw["drop"]))
            out["rope_bwd"] = E.attn_bwd_rope_path(bool(kw["rope"]), kw["D"])
        if fn == "mlp":
            out["mlp"] = E.mlp_path(kw["hidden"], kw["kind"] == "swiglu", kw["up_bias"])
            out["mlp_bwd"] = E.mlp_bwd_path(out["mlp"] == "swiglu_fused", dt, kw["d"], kw["hidden"], kw["B"] * kw["N"])
        if fn in WGRAD_GROUPS:
            out["wgrad"] = {}
            for g, members in WGRAD_GROUPS[fn].items():
                members = [n for n in members if n in names] or ["qkvw"]
                inter = fn == "mlp" and g == "up" and out["mlp"] == "swiglu_fused"
                ina = [n in arena for n in members]
                adjacent = all(ina) and all(lay[a][0] + lay[a][1] == lay[b][0] for a, b in zip(members, members[1:]))
                slab = inter and all(ina) and K.gemm_tn_route(kw["B"] * kw["N"], 2 * kw["hidden"], kw["d"], dt)[1] > 1
                out["wgrad"][g] = E.wgrad_path(ina, inter, slab, adjacent)
        norm_w = "w" if fn == "layernorm" else "ln_w"
        if norm_w in names and fn != "layernorm" or fn == "layernorm":
            norm_b = "b" if fn == "layernorm" else "ln_b"
            out["norm_bwd"] = E.norm_bwd_path(norm_w in arena, norm_b in names, norm_b in arena)
        return out
    finally:
        E.set_compute_dtype(prev)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def defects_for(case):
    """the planted defects that apply to a case"""
    kw, fn, names = case.kw, case.fn, param_names(case)
    out = []
    if fn == "cross" or (fn in ("attn", "mlp") and kw["residual"]):
        out.append("dx_residual")
    sums = {"attn": ["pb", "qkv_b", "ln_w", "ln_b"], "mlp": ["up_b", "down_b", "ln_w", "ln_b"], "cross": ["ln_w", "ln_b"],
            "normlinear": ["b", "ln_w", "ln_b"], "layernorm": ["w", "b"], "patch": ["emb_b", "space"], "mpatch": ["emb_b", "space"],
            "assemble": ["mask_token"]}.get(fn, [])
    out += [("colsum_row", n) for n in sums if n in names]
    if fn == "mlp" and kw["kind"] == "swiglu":
        out.append("up_gate_swap")
    if fn == "attn":
        if not kw["gpt"]:
            out.append("qkv_split")
        if kw["rope"]:
            out += ["no_inverse_rope", "rope_offset"] + (["rope_other_sample"] if kw["rope"] == "per_sample" else [])
        if case.paths["proj"] in ("rope_ps", "ident_ps"):
            out.append("dq_prescale")
        if kw["drop"]:
            out.append("attn_dropout_site")
    if fn in ("attn", "mlp") and kw["drop"]:
        out.append("resid_dropout_bwd")
    if fn == "normlinear" and kw["nout"] % dy_vec(case.dtype):
        out.append("dy_tail")
    if fn == "assemble":
        out.append("pos_token_order")
    if arena_params(case):
        out += ["arena_write", "arena_twice"]
    return out


ALL_DEFECTS = ("dx_residual", "colsum_row", "up_gate_swap", "qkv_split", "no_inverse_rope", "rope_offset", "rope_other_sample", "dq_prescale",
               "resid_dropout_bwd", "attn_dropout_site", "dy_tail", "arena_write", "arena_twice", "pos_token_order")
