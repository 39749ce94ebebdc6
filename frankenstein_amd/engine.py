"""Autograd glue between the nn.Module surface (models/) and the HIP kernels (kernels.py).

Design (MI355X-first, not a translation of the reference's op graph):
  * master parameters stay fp32; kernels consume compute-dtype *shadows* (bf16 or fp32) that are laid
    out for the GEMMs: q/k/v (and w1/w3) concatenated into one [sum N, K] operand, plus a transposed
    copy [K, sum N] so every activation GEMM — forward and dgrad — is the same K-contiguous NT kernel.
  * the unit of autograd is the pre-norm residual branch ("sub-block"):  y = x + f(LN(x)).
    One torch.autograd.Function per branch keeps exactly the tensors the hand-written backward
    needs and fuses the residual-gradient add into the LayerNorm backward kernel.
  * no torch math op is executed on the hot path: only allocation, views and kernel launches.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import dataclasses
import math
import os
import weakref

import torch

from . import kernels as K
from .kernels import NO_MASK

Tensor = torch.Tensor

_COMPUTE_DTYPE = torch.bfloat16
_EPOCH = 0


def set_compute_dtype(dtype) -> None:
    """'bf16' (throughput mode: bf16 operands, fp32 accumulate) or 'fp32' (exact-fp32 MFMA parity mode)."""
    global _COMPUTE_DTYPE
    if isinstance(dtype, str):
        dtype = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}[dtype]
    assert dtype in (torch.bfloat16, torch.float32)
    _COMPUTE_DTYPE = dtype


def compute_dtype() -> torch.dtype:
    return _COMPUTE_DTYPE


def bump_weight_epoch() -> None:
    """Called by the optimizer (which updates masters through raw pointers) to invalidate all shadows."""
    global _EPOCH
    _EPOCH += 1


# --------------------------------------------------------------------------------------------- weight-gradient stream
# dW = dY^T X GEMMs do not feed the rest of the backward: with a flat gradient arena (train_utils.ParamArena) they are
# accumulated straight into the arena (no temporary, no autograd add).  Optionally (FusedAdamW(overlap_wgrad=True) or
# FK_WGRAD_STREAM=1) they run on a SECOND HIP stream beside the dX chain; the optimizer joins that stream before the update and
# DP buckets are all-reduced from it (GradSync).  OFF by default: the large-tile GEMMs are one 128-KiB-LDS block per CU, and two
# such grids from two streams split the CUs unevenly — measured 65 ms steps turning into 80-160 ms ones at random.  (The run-to-run
# differences round 2 saw in this mode were not the stream's doing: compiler-packed fp32 in the RoPE epilogues beside ANY co-resident
# bf16 GEMM, fixed in the build flags — DESIGN.md 5.4, tests/test_coresidency_gpu.py.)
_WGRAD_STREAM = None


def enable_wgrad_stream(on: bool = True):
    global _WGRAD_STREAM
    _WGRAD_STREAM = torch.cuda.Stream() if on else None
    return _WGRAD_STREAM


def wgrad_stream():
    return _WGRAD_STREAM


def _arena_grad(p: Tensor):
    g = p.grad
    return g if (g is not None and getattr(p, "_fk_arena", False) and g.is_contiguous()) else None


def wgrad_path(in_arena: Sequence[bool], swiglu_interleaved: bool = False, slab_ok: bool = False, adjacent: bool = False,
               requires_grad: Optional[Sequence[bool]] = None) -> str:
    """Where wgrad puts the gradients of one row-concatenated weight group (host-side, no GPU).  in_arena: per parameter, whether its
    .grad is a contiguous view of the gradient arena; slab_ok: K.gemm_tn_swiglu_ok of the product; adjacent: the arena views follow
    each other in memory in the order of the group; requires_grad: per parameter (None: all of them do).
      "skip"        no parameter of the group requires grad (a frozen base): no launch, Nones
      "tensors"     one parameter is outside the arena: gemm_tn into a temporary, split (or de-interleaved) and handed to autograd
      "swiglu_slab" gemm_tn_swiglu_: the slab reduction adds the de-interleaved rows to both arena views
      "swiglu_add"  gemm_tn into a temporary, two add2d_ into the arena views
      "adjacent"    gemm_tn accumulates into the arena views as one [sum N, K] matrix
      "split_add"   gemm_tn into a temporary, one add2d_ per parameter"""
    if requires_grad is not None and not any(requires_grad):
        return "skip"
    if not all(in_arena):
        return "tensors"
    if swiglu_interleaved:
        return "swiglu_slab" if slab_ok else "swiglu_add"
    return "adjacent" if adjacent else "split_add"


def norm_bwd_path(gamma_in_arena: bool, has_beta: bool, beta_in_arena: bool) -> str:
    """"arena": norm_bwd accumulates dgamma (and dbeta) straight into the arena views; "tensors": it returns them (host-side, no GPU)."""
    return "arena" if gamma_in_arena and (not has_beta or beta_in_arena) else "tensors"


def wgrad(a: Tensor, b: Tensor, params: Sequence[Tensor], swiglu_interleaved: bool = False):
    """Gradients of the row-concatenated weights `params` = a^T b ([sum N, K], fp32).  Returns a list aligned with params:
    tensors (caller hands them to autograd) or Nones when the result was accumulated directly into the arena (on the
    weight-gradient stream when one is enabled, else on the current stream)."""
    side = _WGRAD_STREAM
    grads = [_arena_grad(p) for p in params]
    in_arena = [g is not None for g in grads]
    first = wgrad_path(in_arena, swiglu_interleaved, requires_grad=[p.requires_grad for p in params])
    if first == "skip":
        return [None] * len(params)
    if first == "tensors":
        dw = K.gemm_tn(a, b)
        if swiglu_interleaved:
            return list(_deinterleave_rows(dw, params[0].shape[0]))
        return _split_rows(dw, params)
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())
        a.record_stream(side)
        b.record_stream(side)
    with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
        Kd = b.shape[1]
        adjacent = all(grads[i + 1].data_ptr() == grads[i].data_ptr() + grads[i].numel() * 4 for i in range(len(grads) - 1))
        path = wgrad_path(in_arena, swiglu_interleaved, swiglu_interleaved and K.gemm_tn_swiglu_ok(a, b, grads[0], grads[1]), adjacent)
        if path == "swiglu_slab":
            K.gemm_tn_swiglu_(a, b, grads[0], grads[1])            # the slab reduction adds the de-interleaved rows to both gradients
        elif path == "swiglu_add":
            dw = K.gemm_tn(a, b)                                   # [2H, K] interleaved rows
            H = params[0].shape[0]
            v = dw.view(H // 4, 8 * Kd)
            K.add2d_(grads[0].view(H // 4, 4 * Kd), v[:, :4 * Kd])
            K.add2d_(grads[1].view(H // 4, 4 * Kd), v[:, 4 * Kd:])
        elif path == "adjacent":
            n = sum(p.shape[0] for p in params)
            out = torch.as_strided(grads[0], (n, Kd), (Kd, 1))
            K.gemm_tn(a, b, out=out, accumulate=True)
        else:
            dw = K.gemm_tn(a, b)
            for g, part in zip(grads, _split_rows(dw, params)):
                K.add2d_(g.view(part.shape), part)
    # autograd still runs the parameters' post-accumulate-grad hooks (GradSync) after this Function returns, once per
    # backward and after the last use of a shared weight, so bucket readiness needs no extra signalling here
    return [None] * len(params)


def norm_bwd(dh: Tensor, x2: Tensor, ln_w: Tensor, ln_b: Optional[Tensor], mean: Tensor, rstd: Tensor, dres: Optional[Tensor] = None,
             kind: int = K.NORM_LAYER):
    """K.norm_bwd whose dgamma / dbeta are accumulated straight into the gradient arena when the parameters live there
    (returns Nones for them: no temporary, no autograd add); plain tensors otherwise."""
    gw = _arena_grad(ln_w)
    gb = _arena_grad(ln_b) if ln_b is not None else None
    if norm_bwd_path(gw is not None, ln_b is not None, gb is not None) == "arena":
        dx, _, _ = K.norm_bwd(dh, x2, ln_w.detach(), mean, rstd, dres=dres, kind=kind, want_beta=ln_b is not None,
                              dgamma=gw.view(-1), dbeta=None if gb is None else gb.view(-1), accumulate=True)
        return dx, None, None
    return K.norm_bwd(dh, x2, ln_w.detach(), mean, rstd, dres=dres, kind=kind, want_beta=ln_b is not None)


# --------------------------------------------------------------------------------------------- shadows
class _Shadow:
    """One compute-dtype weight copy.  `jobs` are the fk_cast_pack_rows calls that fill `tensor` from the masters
    (src, dst view, transpose, rblk, rstride, roff); `params` are weak references (a shadow dies with its model)."""
    __slots__ = ("stamp", "tensor", "jobs", "params", "dtype", "ptrs", "repack", "trained")

    def __init__(self):
        self.stamp, self.tensor, self.jobs, self.params, self.dtype, self.ptrs = None, None, [], (), None, ()
        self.repack = None       # shadows whose layout is not a cast_pack job (convolution weights): callable that refills `tensor` in place
        self.trained = None      # the masters an optimizer must own for refresh_shadows to re-pack this shadow (None: all of `params`)

    def owned_by(self, ids) -> bool:
        return all(id(r()) in ids for r in (self.params if self.trained is None else self.trained))

    def alive(self) -> bool:
        """masters still exist and still live where the pack jobs read them (ParamArena moves parameter storage)"""
        return all(r() is not None and r().data_ptr() == q for r, q in zip(self.params, self.ptrs))

    def current_stamp(self):
        return (_EPOCH, tuple(r()._version for r in self.params))


_SHADOWS: dict = {}
_REFRESH = {"sig": None, "table": None, "njobs": 0, "chunks": 0}


def _run_jobs(ent: "_Shadow") -> None:
    for src, dst, tr, rblk, rstride, roff in ent.jobs:
        if rblk:
            K.cast_pack_rows(src, dst, tr, rblk, rstride, roff)
        else:
            K.cast_pack(src, dst, transpose=tr)


def _shadow_entry(key, params) -> "_Shadow":
    ent = _SHADOWS.get(key)
    if ent is not None and not ent.alive():       # the address was reused by another model's parameter
        ent = None
    if ent is None:
        ent = _SHADOWS[key] = _Shadow()
        # a view (space_embedding.view(C, d), ...) is tracked through its base: the view object dies with the call
        owners = [p._base if p._base is not None else p for p in params]
        ent.params = tuple(weakref.ref(o) for o in owners)
        ent.ptrs = tuple(o.data_ptr() for o in owners)
        ent.dtype = _COMPUTE_DTYPE
    return ent


def shadow(params: Sequence[Tensor], transpose: bool = False, pad_k: int = 0, pad_n: int = 0) -> Tensor:
    """Compute-dtype copy of cat(params, dim=0) ([sum N, K]); transposed -> [K, sum N]; pad_k / pad_n zero-pad
    the K / N extents (16-byte GEMM operand alignment).  1-D params (biases) are concatenated as vectors.
    Re-packed only when a master changed (tensor version counter) or the optimizer bumped the epoch; the optimizer
    re-packs every shadow of its parameters in one launch (refresh_shadows), so in a training loop this is a lookup."""
    dt = _COMPUTE_DTYPE
    key = (tuple((p.data_ptr(), tuple(p.shape)) for p in params), transpose, pad_k, pad_n, dt)
    ent = _shadow_entry(key, params)
    stamp = ent.current_stamp()
    if ent.stamp == stamp:
        return ent.tensor
    if ent.tensor is not None and ent.jobs:        # same masters, new values: re-pack in place
        _run_jobs(ent)
        ent.stamp = stamp
        return ent.tensor
    p0 = params[0]
    for p in params:
        assert p.dtype == torch.float32, "master parameters must be float32 (compute dtype is set with set_compute_dtype)"
    jobs = []
    if p0.dim() == 1:
        n = sum(p.numel() for p in params)
        if dt == torch.float32 and len(params) == 1:
            out = p0.detach()
        else:
            out = torch.empty(n, dtype=dt, device=p0.device)
            off = 0
            for p in params:
                jobs.append((p.detach().view(1, -1), out[off:off + p.numel()].view(1, -1), False, 0, 0, 0))
                off += p.numel()
    else:
        Kd = p0.shape[1]
        kp = max(Kd, pad_k)
        n = sum(p.shape[0] for p in params)
        npad = max(n, pad_n)
        if dt == torch.float32 and len(params) == 1 and not transpose and kp == Kd and npad == n and p0.is_contiguous():
            out = p0.detach()
        else:
            shape = (kp, npad) if transpose else (npad, kp)
            out = (torch.zeros if (kp != Kd or npad != n) else torch.empty)(shape, dtype=dt, device=p0.device)
            off = 0
            for p in params:
                src = p.detach()
                assert src.dim() == 2 and src.shape[1] == Kd and src.is_contiguous()
                dst = out[:Kd, off:off + src.shape[0]] if transpose else out[off:off + src.shape[0], :Kd]
                jobs.append((src, dst, transpose, 0, 0, 0))
                off += src.shape[0]
    ent.jobs, ent.tensor = jobs, out
    _run_jobs(ent)
    ent.stamp = stamp
    return out


def shadow_swiglu(w1: Tensor, w3: Tensor, transpose: bool = False) -> Tensor:
    """Interleaved SwiGLU up-projection shadow: per 4 hidden units, 4 rows of w1 then 4 rows of w3 ([2H, K]; transposed
    [K, 2H]) — the layout the fused GEMM epilogues (fk_gemm_nt_swiglu / fk_gemm_nt_dswiglu) expect."""
    dt = _COMPUTE_DTYPE
    key = (("swiglu", w1.data_ptr(), w3.data_ptr(), tuple(w1.shape)), transpose, dt)
    ent = _shadow_entry(key, (w1, w3))
    stamp = ent.current_stamp()
    if ent.stamp == stamp:
        return ent.tensor
    if ent.tensor is None:
        H, Kd = w1.shape
        assert w3.shape == (H, Kd) and H % 8 == 0 and w1.dtype == torch.float32 and w1.is_contiguous() and w3.is_contiguous()
        out = torch.empty((Kd, 2 * H) if transpose else (2 * H, Kd), dtype=dt, device=w1.device)
        ent.jobs = [(w1.detach(), out, transpose, 4, 8, 0), (w3.detach(), out, transpose, 4, 8, 4)]
        ent.tensor = out
    _run_jobs(ent)
    ent.stamp = stamp
    return ent.tensor


def shadow_lora(w: Tensor, A: Tensor, B: Tensor, scale: float, pad_n: int = 0) -> Tensor:
    """Compute-dtype shadow of the MERGED weight w + scale * (B A) ([N, K], rows zero-padded to pad_n), straight from the three fp32
    masters (fk_lora_merge: the bits of casting the merged fp32 master).  Stamped on the epoch and on the versions of all three
    tensors; refilled IN PLACE, also by refresh_shadows when the optimizer owns A and B (w is frozen and in no optimizer), so a
    captured decode graph sees every step.  Every inference path reads it in place of shadow([w]): no extra launch per step."""
    dt = _COMPUTE_DTYPE
    key = (("lora", w.data_ptr(), A.data_ptr(), B.data_ptr(), tuple(w.shape), tuple(A.shape), float(scale)), pad_n, dt)
    ent = _shadow_entry(key, (w, A, B))
    stamp = ent.current_stamp()
    if ent.stamp == stamp:
        return ent.tensor
    refs = ent.params

    def pack():
        wd, ad, bd = (r().detach() for r in refs)
        n = wd.shape[0]
        if ent.tensor is None:
            ent.tensor = (torch.zeros if pad_n > n else torch.empty)((max(n, pad_n), wd.shape[1]), dtype=dt, device=wd.device)
        K.lora_merge(wd, ad, bd, scale, out=ent.tensor[:n])      # in place: the storage a captured GEMM reads stays the same

    ent.repack, ent.trained = pack, refs[1:]
    pack()
    ent.stamp = stamp
    return ent.tensor


def refresh_shadows(params: Sequence[Tensor]) -> None:
    """Re-pack, in ONE launch (fk_cast_pack_multi), every shadow built so far whose masters all belong to `params` — called by
    the optimizer right after it updated the masters (one launch per step instead of one or two per weight)."""
    ids = {id(p) for p in params}
    for k in [k for k, e in _SHADOWS.items() if not e.alive()]:
        del _SHADOWS[k]
    # shadows with their own in-place re-pack (convolution weights): refreshed here too, so that a captured graph, which keeps
    # reading the shadow's storage, sees every optimizer step (they used to be rebuilt lazily into NEW storage by the eager forward only)
    for e in _SHADOWS.values():
        if e.repack is not None and e.tensor is not None and e.dtype == _COMPUTE_DTYPE and e.owned_by(ids):
            e.repack()
            e.stamp = e.current_stamp()
    ents = [e for e in _SHADOWS.values()
            if e.jobs and e.dtype == _COMPUTE_DTYPE and e.tensor.is_cuda and all(id(r()) in ids for r in e.params)]
    if not ents:
        return
    sig = tuple(id(e) for e in ents)
    if _REFRESH["sig"] != sig:
        import numpy as np
        rec = np.dtype([("src", "<u8"), ("dst", "<u8"), ("lds", "<i8"), ("ldd", "<i8"), ("rows", "<i4"), ("cols", "<i4"),
                        ("transpose", "<i4"), ("rblk", "<i4"), ("rstride", "<i4"), ("roff", "<i4"), ("chunk_begin", "<i8")])
        assert rec.itemsize == 64
        rows, chunks = [], 0
        for e in ents:
            for src, dst, tr, rblk, rstride, roff in e.jobs:
                r, c = src.shape
                rows.append((src.data_ptr(), dst.data_ptr(), src.stride(0), dst.stride(0), r, c, int(tr), rblk, rstride, roff, chunks))
                chunks += ((r + 31) // 32) * ((c + 31) // 32) if tr else (r * c + 1023) // 1024
        tab = torch.from_numpy(np.array(rows, dtype=rec).view(np.uint8).copy()).to(ents[0].tensor.device)
        _REFRESH.update(sig=sig, table=tab, njobs=len(rows), chunks=chunks, ents=ents)
    K.cast_pack_multi(_REFRESH["table"], _REFRESH["njobs"], _REFRESH["chunks"], _COMPUTE_DTYPE)
    for e in ents:
        e.stamp = e.current_stamp()


def _deinterleave_rows(t: Tensor, H: int):
    """[2H, K] fp32 in the interleaved row order -> (rows of w1, rows of w3), each [H, K] contiguous."""
    Kd = t.shape[1]
    a = torch.empty((H, Kd), dtype=t.dtype, device=t.device)
    b = torch.empty((H, Kd), dtype=t.dtype, device=t.device)
    v = t.view(H // 4, 8 * Kd)
    K.copy2d(v[:, :4 * Kd], a.view(H // 4, 4 * Kd))
    K.copy2d(v[:, 4 * Kd:], b.view(H // 4, 4 * Kd))
    return a, b


def _split_rows(t: Tensor, params: Sequence[Tensor]) -> List[Tensor]:
    out, off = [], 0
    for p in params:
        n = p.shape[0]
        out.append(t[off:off + n].view(p.shape))
        off += n
    return out


def to_compute(x: Tensor) -> Tensor:
    """fp32 / bf16 activation -> compute dtype (kernel cast, no autograd: inputs only)."""
    if x.dtype == _COMPUTE_DTYPE:
        return x.contiguous()
    return K.cast(x.contiguous(), _COMPUTE_DTYPE)


# --------------------------------------------------------------------------------------------- rope spec
_ROPE_PAIRS: dict = {}


class Rope:
    """fp32 (cos, sin) table [Tc, D/2, 2] (or per-sample [B, Tc, D/2, 2]); the LAST T rows are used
    (models/brainformer.py:80,82)."""
    __slots__ = ("table", "_src")

    def __init__(self, cache: Tensor):
        t = torch.view_as_real(cache) if cache.is_complex() else cache
        assert t.dtype == torch.float32 and t.shape[-1] == 2
        self.table = t.contiguous()
        self._src = cache

    def pos_off(self, T: int) -> int:
        return self.table.shape[-3] - T

    def pair(self, c: float):
        """(table, table * c) as the two halves of ONE allocation: the second is what fk_gemm_nt_rope rotates the query columns
        with, so that Q leaves the projection multiplied by c = softmax_scale * log2(e) (FK_ATTN_Q_PRESCALED).  Cached per cache
        tensor (the model hands the same tensor to every layer); the entry dies with the tensor."""
        src, key = self._src, id(self._src)
        ent = _ROPE_PAIRS.get(key)
        stamp = (src._version, float(c), src.data_ptr())
        if ent is not None and ent[0]() is src and ent[1] == stamp:
            return ent[2][0], ent[2][1]
        both = torch.stack([self.table, self.table * float(c)]).contiguous()
        _ROPE_PAIRS[key] = (weakref.ref(src, lambda _r, k=key: _ROPE_PAIRS.pop(k, None)), stamp, both)
        return both[0], both[1]


_IDENT_PAIRS: dict = {}


def identity_pair(D: int, c: float, device):
    """(table, q_table) for attention blocks WITHOUT RoPE (SimpleMAE's / MAE's decoder, GPT-2 at head_dim 64): eight identical rows of
    (cos, sin) = (1, 0) and (c, 0).  Through fk_gemm_nt_rope's epilogue the key columns stay bit-exact (x * 1 - y * 0) and the query
    columns leave the projection as c * q with one rounding, i.e. pre-scaled for the lean attention kernels (FK_ATTN_Q_PRESCALED) —
    without it those blocks ran the generic kernels (SimpleMAE decoder at B = 32: 208 + 157 + 160 us per layer for 18 GFLOP)."""
    key = (D, float(c), str(device))
    ent = _IDENT_PAIRS.get(key)
    if ent is None:
        one = torch.zeros((8, D // 2, 2), dtype=torch.float32)
        one[..., 0] = 1.0
        ent = _IDENT_PAIRS[key] = torch.stack([one, one * float(c)]).contiguous().to(device)
    return ent[0], ent[1]


def _attn_prescale(D: int) -> bool:
    """Queries pre-scaled by scale * log2(e) in the projection epilogue + the lean attention kernels: bf16, head_dim 64."""
    return _COMPUTE_DTYPE == torch.bfloat16 and D == 64


def attn_proj_path(B: int, N: int, H: int, D: int, has_rope: bool, mask_kind: int, has_dropout: bool) -> str:
    """The QKV projection AttnBranch.forward runs for B x N tokens, H heads of width D, in the current compute dtype (host-side, no GPU):
      "rope_ps"    gemm_nt_rope, queries rotated with the pre-scaled table (lean attention kernels)
      "rope"       gemm_nt_rope, one table (fp32 mode, head_dim != 64, dense masks, dropout)
      "ident_ps"   no RoPE: gemm_nt_rope with the identity pair, queries pre-scaled
      "plain"      no RoPE: gemm_nt
      "plain_rope" gemm_nt, then rope_ in place (head widths the fused epilogue does not take)"""
    HD = H * D
    ps = _attn_prescale(D) and mask_kind != K.MASK_DENSE and not has_dropout     # dense masks / dropout: the generic kernels
    if has_rope and D % 8 == 0 and (3 * HD) % 8 == 0:     # RoPE fused into the projection epilogue
        return "rope_ps" if ps else "rope"
    if (not has_rope and N >= 64 and (B * N) % 8 == 0 and (3 * HD) % 8 == 0 and ps
            and os.environ.get("FK_ATTN_NO_IDENT_PRESCALE") is None):
        return "ident_ps"
    return "plain_rope" if has_rope else "plain"


def attn_bwd_rope_path(has_rope: bool, D: int) -> Optional[str]:
    """How AttnBranch.backward un-rotates dQ / dK: "fused" into attn_bwd's stores, "kernel" = rope_(conj) afterwards, None without RoPE."""
    if not has_rope:
        return None
    return "fused" if D % 4 == 0 else "kernel"


# --------------------------------------------------------------------------------------------- dropout
# nn.Dropout / SDPA dropout_p of the GPT-2 decoder in training mode (models/gpt2_model.py:40,64,75,85,91,129).  No mask tensor exists:
# every application is (p, seed words, site) and the kernels regenerate keep / drop from the element index (include/franken_hip.h,
# fk_dropout).  The MASTER seed words live on the device — [torch.initial_seed(), a step counter advanced once per forward by
# dropout_begin()] — so a captured training step draws new masks on every replay; `site` numbers the applications within one forward.
# Every forward works on its own SNAPSHOT of the two words (one 8-byte device copy, captured in graphs too): a backward that runs after
# another training-mode forward (two forwards, then (l1 + l2).backward(); a recompute) regenerates the masks ITS forward drew, like
# torch's dropout.  No words tensor is ever replaced: a captured graph holds raw pointers to them, so a new seed is written in place.
_DROP_WORDS: dict = {}
_DROP_CUR: dict = {}
_DROP_SITE = [0]


def dropout_words(device) -> Tensor:
    """The master [seed, step] words of `device` (int32, device memory; the same tensor for the life of the process)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    seed = torch.initial_seed() & 0x7FFFFFFF
    ent = _DROP_WORDS.get(device)
    if ent is None:
        ent = _DROP_WORDS[device] = [seed, torch.tensor([seed, 0], dtype=torch.int32, device=device)]
    elif ent[0] != seed and not torch.cuda.is_current_stream_capturing():
        ent[0] = seed
        ent[1].copy_(torch.tensor([seed, 0], dtype=torch.int32))        # a new torch.manual_seed: restart the stream, in place
    return ent[1]


def dropout_begin(device) -> None:
    """Start of a training forward with dropout > 0: the next step's masks (master step word + 1 on the device), this forward's
    snapshot of the words, sites numbered from 0."""
    words = dropout_words(device)
    words[1:].add_(1)
    _DROP_CUR[words.device] = words.clone()
    _DROP_SITE[0] = 0


def dropout_snapshot(device) -> Tensor:
    """The words the current forward draws with (dropout_begin's snapshot; the master words before any forward began)."""
    words = dropout_words(device)
    return _DROP_CUR.get(words.device, words)


def dropout_site() -> int:
    _DROP_SITE[0] += 1
    return _DROP_SITE[0] - 1


def drop_spec(p: float, device, n_sites: int):
    """(p, seed words, site, ...) for one module call, or None when p == 0."""
    if not p:
        return None
    assert 0.0 < p < 1.0, f"dropout p = {p}"
    return (float(p), dropout_snapshot(device)) + tuple(dropout_site() for _ in range(n_sites))


class Dropout(torch.autograd.Function):
    """y = nn.Dropout(p)(x) in training mode (embedding dropout, models/gpt2_model.py:129,190)."""

    @staticmethod
    def forward(ctx, x, drop):
        ctx.drop = drop
        return K.dropout(x.contiguous(), drop[0], drop[1], drop[2])

    @staticmethod
    def backward(ctx, dy):
        d = ctx.drop
        return K.dropout(dy.contiguous(), d[0], d[1], d[2]), None


# --------------------------------------------------------------------------------------------- signal augmentation
# Training-time perturbation of the neural features, drawn inside the patch tokeniser (fk_augment_patchify; the rule is in
# include/franken_hip.h and restated in tests/augment_ref.py).  Like dropout it owns a [seed, step] word pair on the device, a stream of
# its own (advancing dropout does not move the augmentation and vice versa): augment_begin() adds 1 to the step word on the device, so a
# captured training step draws fresh noise on every replay.  The tokens are saved for the backward, so nothing is ever regenerated and
# no snapshot of the words is needed.
_AUG_WORDS: dict = {}


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """The knobs of the signal augmentation; all zero = off.  white_sd / offset_sd: standard deviations of the per-frame white noise and
    of the per-trial channel offset (in units of the z-scored signal); chan_drop_p: probability that an electrode is zeroed for a trial;
    time_shift S: a shift of -S .. S frames per trial; n_time_masks spans of 0 .. time_mask_len frames are zeroed; keep_padding: all-zero
    frames (padding) receive no noise."""
    white_sd: float = 0.0
    offset_sd: float = 0.0
    chan_drop_p: float = 0.0
    time_shift: int = 0
    n_time_masks: int = 0
    time_mask_len: int = 0
    keep_padding: bool = True

    @property
    def active(self) -> bool:
        return bool(self.white_sd > 0 or self.offset_sd > 0 or self.chan_drop_p > 0 or self.time_shift > 0
                    or (self.n_time_masks > 0 and self.time_mask_len > 0))

    @classmethod
    def from_model_config(cls, config) -> "AugmentConfig":
        """from the aug_* fields of MAEConfig / SimpleEncoderConfig (a config without them: everything off)"""
        g = lambda name: getattr(config, name, 0) or 0
        return cls(float(g("aug_white_sd")), float(g("aug_offset_sd")), float(g("aug_chan_drop")), int(g("aug_time_shift")),
                   int(g("aug_time_masks")), int(g("aug_time_mask_len")))


def augment_seed(initial_seed: int, rank: int = 0) -> int:
    """The seed word: data-parallel ranks hold different samples and must not draw the same noise.  31 bits (an int32 tensor holds it)."""
    return (int(initial_seed) + 0x9E3779B9 * int(rank)) & 0x7FFFFFFF


def _dist_rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def augment_words(device) -> Tensor:
    """The [seed, step] words of `device` (int32, device memory; the same tensor for the life of the process).  A new torch.manual_seed
    restarts the stream in place, never while capturing (a captured graph holds the tensor's address)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    seed = augment_seed(torch.initial_seed(), _dist_rank())
    ent = _AUG_WORDS.get(device)
    if ent is None:
        ent = _AUG_WORDS[device] = [seed, torch.tensor([seed, 0], dtype=torch.int32, device=device)]
    elif ent[0] != seed and not torch.cuda.is_current_stream_capturing():
        ent[0] = seed
        ent[1].copy_(torch.tensor([seed, 0], dtype=torch.int32))
    return ent[1]


def augment_begin(device) -> Tensor:
    """Start of a training forward with an active augmentation: step word + 1 on the device (inside a captured graph too).  Returns the words."""
    words = augment_words(device)
    words[1:].add_(1)
    return words


def augment_tokens(x: Tensor, P: int, ldp: int, dtype: torch.dtype, cfg: AugmentConfig, words: Optional[Tensor] = None) -> Tensor:
    """to_patches(augment(x)) [B * (T / P) * C, ldp] drawn at the CURRENT step word (the caller has called augment_begin)"""
    xin = x if x.dtype == torch.float32 else K.cast(x.contiguous(), torch.float32)
    xin = xin.contiguous()
    return K.augment_patchify(xin, P, ldp, dtype, cfg, augment_words(xin.device) if words is None else words)


def augment_signal(x: Tensor, cfg: AugmentConfig, words: Optional[Tensor] = None) -> Tensor:
    """The augmented [B, T, C] signal itself in fp32 (the kernel's P = 1 mode), drawn at the current step word: bit for bit what the
    fused tokeniser patchifies at the same words."""
    B, T, Cn = x.shape
    return augment_tokens(x, 1, 1, torch.float32, cfg, words).view(B, T, Cn)


# --------------------------------------------------------------------------------------------- functions
def _lora_add(x2: Tensor, A: Tensor, B: Tensor, scale: float, y: Tensor, q_cols: int = 0, q_scale: float = 1.0) -> Tensor:
    """y += scale * colscale * ((x2 A^T) B^T) in ONE launch (fk_lora_fwd, in place on y); returns u = x2 A^T for the backward"""
    _, u = K.lora_fwd(x2, shadow([A]), shadow([B]), scale, res=y, out=y, q_cols=q_cols, q_scale=q_scale)
    return u


def _lora_backward(dy2: Tensor, x2: Tensor, u: Tensor, A: Tensor, B: Tensor, scale: float, dx: Tensor):
    """The adapter's share of a Linear's backward: dx += scale * (dy2 B) A in one launch (fk_lora_fwd on the transposed shadows), then
    dA, dB in one fk_lora_wgrad — accumulated straight into the gradient arena when both live there (Nones), tensors otherwise."""
    _, du = K.lora_fwd(dy2, shadow([B], transpose=True), shadow([A], transpose=True), scale, res=dx, out=dx)
    gA, gB = _arena_grad(A), _arena_grad(B)
    if gA is not None and gB is not None:
        K.lora_wgrad(dy2, u, du, x2, scale, dA=gA, dB=gB, accumulate=True)
        return None, None
    return K.lora_wgrad(dy2, u, du, x2, scale)


class AttnBranch(torch.autograd.Function):
    """y = [x +] proj(SDPA(rope(q), rope(k), v)) with q,k,v = Linear([LN](x));  one pre-norm attention branch.

    Reference: Block.forward attention half (models/brainformer.py:243 with :147-173) and
    gpt2 Block (models/gpt2_model.py:104 with :52-76)."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, pw, pb, qkv_b, spec, *qkv_w):
        return AttnBranch.run_forward(ctx, x, ln_w, ln_b, pw, pb, qkv_b, spec, qkv_w, None)

    @staticmethod
    def backward(ctx, dy):
        return AttnBranch.run_backward(ctx, dy)[0]

    @staticmethod
    def run_forward(ctx, x, ln_w, ln_b, pw, pb, qkv_b, spec, qkv_w, lora):
        """the body of forward; lora = (scale, A_qkv, B_qkv, A_proj, B_proj), either pair None, for the adapted form (AttnBranchLora):
        the correction joins c_attn's output with the query scale applied, and c_proj's output before the residual dropout"""
        H, D, mask, rope, residual, eps, nkind = spec[:7]
        drop = spec[7] if len(spec) > 7 else None       # (p, seed words, site of the attention dropout, site of the residual dropout)
        B, N, d = x.shape
        M = B * N
        x2 = x.view(M, d)
        has_ln = ln_w is not None
        if has_ln:
            h, mean, rstd = K.norm_fwd(x2, ln_w.detach(), None if ln_b is None else ln_b.detach(), eps, nkind)
        else:
            h, mean, rstd = x2, None, None
        HD = H * D
        bq = None if qkv_b is None else shadow([qkv_b])
        path = attn_proj_path(B, N, H, D, rope is not None, mask.kind, drop is not None)
        prescale = path in ("rope_ps", "ident_ps")
        if path == "rope_ps":                         # RoPE fused into the projection epilogue, queries pre-scaled
            tab, qtab = rope.pair((1.0 / math.sqrt(D)) * 1.4426950408889634)
            qkv = K.gemm_nt_rope(h, shadow(qkv_w), bq, tab, N, rope.pos_off(N), D, 2 * HD, q_cols=HD, q_table=qtab)
        elif path == "rope":
            qkv = K.gemm_nt_rope(h, shadow(qkv_w), bq, rope.table, N, rope.pos_off(N), D, 2 * HD)
        elif path == "ident_ps":
            # no RoPE, but the lean kernels want pre-scaled queries: the same epilogue with an identity "rotation" (identity_pair)
            tab, qtab = identity_pair(D, (1.0 / math.sqrt(D)) * 1.4426950408889634, x.device)
            qkv = K.gemm_nt_rope(h, shadow(qkv_w), bq, tab, 8, 0, D, 2 * HD, q_cols=HD, q_table=qtab)
        else:
            qkv = K.gemm_nt(h, shadow(qkv_w), bias=bq)
        u_q = u_p = None
        if lora is not None and lora[1] is not None:
            assert rope is None, "adapters on a rotated projection are not supported (GPT-2 branches have no RoPE)"
            u_q = _lora_add(h, lora[1], lora[2], lora[0], qkv, HD if prescale else 0, (1.0 / math.sqrt(D)) * 1.4426950408889634)
        qkv3 = qkv.view(B, N, 3 * HD)
        if path == "plain_rope":
            K.rope_(qkv3, 2 * H, D, rope.table, rope.pos_off(N))
        q, k, v = (qkv3[..., i * HD:(i + 1) * HD].unflatten(-1, (H, D)) for i in range(3))
        o, lse = K.attn_fwd(q, k, v, mask, q_prescaled=prescale, dropout=None if drop is None else drop[:3])
        if drop is None:
            y = K.gemm_nt(o.view(M, HD), shadow([pw]), bias=None if pb is None else shadow([pb]),
                          residual=x2 if residual else None)
            if lora is not None and lora[3] is not None:     # x + c_proj(o) + delta: added to the finished row, one launch
                u_p = _lora_add(o.view(M, HD), lora[3], lora[4], lora[0], y)
        else:                                           # x + resid_dropout(c_proj(y))  (models/gpt2_model.py:75,104)
            y = K.gemm_nt(o.view(M, HD), shadow([pw]), bias=None if pb is None else shadow([pb]))
            if lora is not None and lora[3] is not None:     # x + drop(c_proj(o) + delta)
                u_p = _lora_add(o.view(M, HD), lora[3], lora[4], lora[0], y)
            K.dropout(y, drop[0], drop[1], drop[3], residual=x2 if residual else None, out=y)
        ctx.spec, ctx.has_ln, ctx.nw, ctx.prescale = spec, has_ln, len(qkv_w), prescale
        ctx.flags = (ln_b is not None, pb is not None, qkv_b is not None)
        ctx.ln_b = ln_b
        ctx.lora_scale = None if lora is None else lora[0]
        extra = () if lora is None else (lora[1], lora[2], lora[3], lora[4], u_q, u_p)
        ctx.save_for_backward(x, ln_w, pw, *qkv_w, h if has_ln else None, mean, rstd, qkv, o, lse, *extra)
        return y.view(B, N, -1)

    @staticmethod
    def run_backward(ctx, dy):
        """the body of backward -> (the gradients of forward's inputs, (dA_qkv, dB_qkv, dA_proj, dB_proj) of the adapted form or None)"""
        H, D, mask, rope, residual, eps, nkind = ctx.spec[:7]
        drop = ctx.spec[7] if len(ctx.spec) > 7 else None
        sv = ctx.saved_tensors
        x, ln_w, pw = sv[0], sv[1], sv[2]
        qkv_w = sv[3:3 + ctx.nw]
        h, mean, rstd, qkv, o, lse = sv[3 + ctx.nw:9 + ctx.nw]
        lora = sv[9 + ctx.nw:] if ctx.lora_scale is not None else None
        dlora = [None] * 4
        has_lnb, has_pb, has_qb = ctx.flags
        has_pb, has_qb = has_pb and ctx.needs_input_grad[4], has_qb and ctx.needs_input_grad[5]     # a frozen bias: no column sum
        B, N, d = x.shape
        M, HD = B * N, H * D
        x2 = x.view(M, d)
        if h is None:
            h = x2
        dy2 = dy.contiguous().view(M, -1)
        dyp = dy2 if drop is None else K.dropout(dy2, drop[0], drop[1], drop[3])        # the gradient behind the residual dropout
        do = K.gemm_nt(dyp, shadow([pw], transpose=True))
        if lora is not None and lora[2] is not None:
            dlora[2], dlora[3] = _lora_backward(dyp, o.view(M, HD), lora[5], lora[2], lora[3], ctx.lora_scale, do)
        (dpw,) = wgrad(dyp, o.view(M, HD), [pw])
        dpb = K.colsum(dyp) if has_pb else None
        dqkv = torch.empty_like(qkv)
        qkv3, dqkv3 = qkv.view(B, N, 3 * HD), dqkv.view(B, N, 3 * HD)
        q, k, v = (qkv3[..., i * HD:(i + 1) * HD].unflatten(-1, (H, D)) for i in range(3))
        dq, dk, dv = (dqkv3[..., i * HD:(i + 1) * HD].unflatten(-1, (H, D)) for i in range(3))
        rpath = attn_bwd_rope_path(rope is not None, D)
        if rpath == "fused":                      # inverse RoPE fused into the dQ / dK stores
            K.attn_bwd(q, k, v, o, do.view(B, N, H, D), lse, dq, dk, dv, mask, rope_table=rope.table, rope_off=rope.pos_off(N),
                       q_prescaled=ctx.prescale, dropout=None if drop is None else drop[:3])
        else:
            K.attn_bwd(q, k, v, o, do.view(B, N, H, D), lse, dq, dk, dv, mask, q_prescaled=ctx.prescale, dropout=None if drop is None else drop[:3])
            if rpath == "kernel":
                K.rope_(dqkv3, 2 * H, D, rope.table, rope.pos_off(N), conj=True)
        dh = K.gemm_nt(dqkv, shadow(qkv_w, transpose=True))
        if lora is not None and lora[0] is not None:     # dqkv is the gradient w.r.t. the UNSCALED q | k | v: no column scale here
            dlora[0], dlora[1] = _lora_backward(dqkv, h, lora[4], lora[0], lora[1], ctx.lora_scale, dh)
        dws = wgrad(dqkv, h, list(qkv_w))
        dqb = K.colsum(dqkv) if has_qb else None
        if ctx.has_ln:
            dx, dg, db = norm_bwd(dh, x2, ln_w, ctx.ln_b, mean, rstd, dres=dy2 if residual else None, kind=nkind)
        else:
            dx, dg, db = (K.add(dh, dy2) if residual else dh), None, None
        return (dx.view(B, N, d), dg, db, dpw, dpb, dqb, None, *dws), (None if lora is None else dlora)


class AttnBranchLora(torch.autograd.Function):
    """AttnBranch with low-rank adapters on c_attn and / or the attention c_proj (csrc/lora.hip); the base GEMMs, their routes and the
    frozen-parameter rules are AttnBranch's.  lora = (A_qkv [r, d], B_qkv [3 H D, r], A_proj [r, H D], B_proj [d, r]), a pair may be
    None; scale = alpha / r.  The adapters are inputs, so autograd sees them."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, pw, pb, qkv_b, spec, scale, a_qkv, b_qkv, a_proj, b_proj, *qkv_w):
        return AttnBranch.run_forward(ctx, x, ln_w, ln_b, pw, pb, qkv_b, spec, qkv_w, (scale, a_qkv, b_qkv, a_proj, b_proj))

    @staticmethod
    def backward(ctx, dy):
        g, dl = AttnBranch.run_backward(ctx, dy)
        return (*g[:7], None, *dl, *g[7:])


class CrossAttnBranch(torch.autograd.Function):
    """y = x + proj(SDPA(q = Wq LN(x), k = Wk ctx, v = Wv ctx))  (models/brainformer.py:262 with :198-219)."""

    @staticmethod
    def forward(ctx, x, context, ln_w, ln_b, qw, kw, vw, pw, spec):
        H, D, mask, eps = spec
        B, T, d = x.shape
        Nc = context.shape[1]
        HD = H * D
        x2, c2 = x.view(B * T, d), context.view(B * Nc, d)
        h, mean, rstd = K.norm_fwd(x2, ln_w.detach(), ln_b.detach(), eps)
        ctx.ln_b = ln_b
        q = K.gemm_nt(h, shadow([qw]))
        kv = K.gemm_nt(c2, shadow([kw, vw]))
        kv3 = kv.view(B, Nc, 2 * HD)
        o, lse = K.attn_fwd(q.view(B, T, H, D), kv3[..., :HD].unflatten(-1, (H, D)), kv3[..., HD:].unflatten(-1, (H, D)), mask)
        y = K.gemm_nt(o.view(B * T, HD), shadow([pw]), residual=x2)
        ctx.spec = spec
        ctx.save_for_backward(x, context, ln_w, qw, kw, vw, pw, h, mean, rstd, q, kv, o, lse)
        return y.view(B, T, d)

    @staticmethod
    def backward(ctx, dy):
        H, D, mask, eps = ctx.spec
        x, context, ln_w, qw, kw, vw, pw, h, mean, rstd, q, kv, o, lse = ctx.saved_tensors
        B, T, d = x.shape
        Nc, HD = context.shape[1], H * D
        x2, c2 = x.view(B * T, d), context.view(B * Nc, d)
        dy2 = dy.contiguous().view(B * T, d)
        do = K.gemm_nt(dy2, shadow([pw], transpose=True))
        (dpw,) = wgrad(dy2, o.view(B * T, HD), [pw])
        dkv = torch.empty_like(kv)
        dq = torch.empty_like(q)
        kv3, dkv3 = kv.view(B, Nc, 2 * HD), dkv.view(B, Nc, 2 * HD)
        K.attn_bwd(q.view(B, T, H, D), kv3[..., :HD].unflatten(-1, (H, D)), kv3[..., HD:].unflatten(-1, (H, D)), o,
                   do.view(B, T, H, D), lse, dq.view(B, T, H, D), dkv3[..., :HD].unflatten(-1, (H, D)),
                   dkv3[..., HD:].unflatten(-1, (H, D)), mask)
        dh = K.gemm_nt(dq, shadow([qw], transpose=True))
        (dqw,) = wgrad(dq, h, [qw])
        dctx = K.gemm_nt(dkv, shadow([kw, vw], transpose=True))
        dkw, dvw = wgrad(dkv, c2, [kw, vw])
        dx, dg, db = norm_bwd(dh, x2, ln_w, ctx.ln_b, mean, rstd, dres=dy2)
        return dx.view(B, T, d), dctx.view(B, Nc, d), dg, db, dqw, dkw, dvw, dpw, None


_MLP_BWD_FUSED = os.environ.get("FK_MLP_BWD_FUSED", "1") != "0"


def mlp_path(hidden: int, has_gate: bool, has_up_bias: bool) -> str:
    """MlpBranch.forward's up-projection (host-side, no GPU): "swiglu_fused" = gemm_nt_swiglu on the interleaved shadow, "swiglu" =
    gemm_nt + swiglu_fwd, "gelu" = gemm_nt + gelu_fwd."""
    if not has_gate:
        return "gelu"
    return "swiglu_fused" if not has_up_bias and hidden % 8 == 0 else "swiglu"


def mlp_bwd_path(fused: bool, dtype, d: int, hidden: int, rows: int) -> str:
    """MlpBranch.backward's data-gradient chain (host-side, no GPU): "one_launch" = mlp_bwd_fused, "dswiglu" = gemm_nt_dswiglu + gemm_nt,
    "plain" = gemm_nt, swiglu_bwd / gelu_bwd, gemm_nt."""
    if not fused:
        return "plain"
    # 128 tokens per workgroup: below ~256 workgroups the two tiled GEMMs fill the chip better
    if (_MLP_BWD_FUSED and dtype == torch.bfloat16 and d == 384 and hidden % 32 == 0 and rows >= 32768
            and rows * (2 * hidden) * 2 < 2 ** 32):
        return "one_launch"
    return "dswiglu"


class MlpBranch(torch.autograd.Function):
    """y = [x +] W2 act(W1 [LN](x)):  SwiGLU (w1,w3 -> silu*gate -> w2, models/brainformer.py:115-124,244) when
    ``gate_w`` is given, GELU-erf MLP with biases (models/gpt2_model.py:87-92,105) otherwise."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, up_w, up_b, gate_w, down_w, down_b, spec):
        return MlpBranch.run_forward(ctx, x, ln_w, ln_b, up_w, up_b, gate_w, down_w, down_b, spec, None)

    @staticmethod
    def backward(ctx, dy):
        return MlpBranch.run_backward(ctx, dy)[0]

    @staticmethod
    def run_forward(ctx, x, ln_w, ln_b, up_w, up_b, gate_w, down_w, down_b, spec, lora):
        """the body of forward; lora = (scale, A_up, B_up, A_down, B_down), either pair None, for the adapted form (MlpBranchLora, the
        GELU MLP only): the correction joins c_fc's pre-activation before the GELU and c_proj's output before the dropout"""
        residual, eps, nkind = spec[:3]
        drop = spec[3] if len(spec) > 3 else None       # (p, seed words, site): dropout on the down-projection's output
        shp = x.shape
        d = shp[-1]
        x2 = x.reshape(-1, d)
        has_ln = ln_w is not None
        if has_ln:
            h, mean, rstd = K.norm_fwd(x2, ln_w.detach(), None if ln_b is None else ln_b.detach(), eps, nkind)
        else:
            h, mean, rstd = x2, None, None
        fused = mlp_path(up_w.shape[0], gate_w is not None, up_b is not None) == "swiglu_fused"
        u_up = u_down = None
        if fused:    # up-projection + SwiGLU in one kernel (interleaved hidden layout)
            a, g = K.gemm_nt_swiglu(h, shadow_swiglu(up_w, gate_w))
        else:
            ups = [up_w] if gate_w is None else [up_w, gate_w]
            a = K.gemm_nt(h, shadow(ups), bias=None if up_b is None else shadow([up_b]))
            if lora is not None and lora[1] is not None:
                assert gate_w is None, "adapters are built for the GELU MLP"
                u_up = _lora_add(h, lora[1], lora[2], lora[0], a)
            g = K.gelu_fwd(a) if gate_w is None else K.swiglu_fwd(a)
        assert lora is None or not fused, "adapters are built for the GELU MLP"
        if drop is None:
            y = K.gemm_nt(g, shadow([down_w]), bias=None if down_b is None else shadow([down_b]),
                          residual=x2 if residual else None)
            if lora is not None and lora[3] is not None:     # x + c_proj(g) + delta: added to the finished row, one launch
                u_down = _lora_add(g, lora[3], lora[4], lora[0], y)
        else:                                           # x + dropout(c_proj(gelu(c_fc(x))))  (models/gpt2_model.py:87-92,105)
            y = K.gemm_nt(g, shadow([down_w]), bias=None if down_b is None else shadow([down_b]))
            if lora is not None and lora[3] is not None:     # x + drop(c_proj(g) + delta)
                u_down = _lora_add(g, lora[3], lora[4], lora[0], y)
            K.dropout(y, drop[0], drop[1], drop[2], residual=x2 if residual else None, out=y)
        ctx.spec, ctx.has_ln, ctx.fused = spec, has_ln, fused
        ctx.flags = (ln_b is not None, up_b is not None, gate_w is not None, down_b is not None)
        ctx.ln_b = ln_b
        ctx.lora_scale = None if lora is None else lora[0]
        extra = () if lora is None else (lora[1], lora[2], lora[3], lora[4], u_up, u_down)
        ctx.save_for_backward(x, ln_w, up_w, gate_w, down_w, h if has_ln else None, mean, rstd, a, g, *extra)
        return y.view(*shp[:-1], y.shape[-1])

    @staticmethod
    def run_backward(ctx, dy):
        """the body of backward -> (the gradients of forward's inputs, (dA_up, dB_up, dA_down, dB_down) of the adapted form or None)"""
        residual, eps, nkind = ctx.spec[:3]
        drop = ctx.spec[3] if len(ctx.spec) > 3 else None
        x, ln_w, up_w, gate_w, down_w, h, mean, rstd, a, g = ctx.saved_tensors[:10]
        lora = ctx.saved_tensors[10:] if ctx.lora_scale is not None else None
        dlora = [None] * 4
        has_lnb, has_ub, gated, has_db = ctx.flags
        has_ub, has_db = has_ub and ctx.needs_input_grad[4], has_db and ctx.needs_input_grad[7]     # a frozen bias: no column sum
        shp = x.shape
        d = shp[-1]
        x2 = x.reshape(-1, d)
        if h is None:
            h = x2
        dy2 = dy.contiguous().view(x2.shape[0], -1)
        ups = [up_w, gate_w] if gated else [up_w]
        dyd = dy2 if drop is None else K.dropout(dy2, drop[0], drop[1], drop[2])         # the gradient behind the dropout
        (ddown,) = wgrad(dyd, g, [down_w])
        ddb = K.colsum(dyd) if has_db else None
        bpath = mlp_bwd_path(ctx.fused, dyd.dtype, d, g.shape[1], dyd.shape[0])
        if bpath == "one_launch":
            # both products of the data-gradient chain in ONE attention-shaped launch, dh13 handed over in registers: the same bits as the
            # two launches below, -0.3 ... -0.4 ms per cfg2 step; FK_MLP_BWD_FUSED=0 keeps the two launches
            da, dh = K.mlp_bwd_fused(dyd, shadow([down_w], transpose=True), a, shadow_swiglu(up_w, gate_w, transpose=True))
            dups = wgrad(da, h, [up_w, gate_w], swiglu_interleaved=True)
        elif bpath == "dswiglu":   # down-projection dgrad + SwiGLU backward in one kernel; dg is never materialised
            da = K.gemm_nt_dswiglu(dyd, shadow([down_w], transpose=True), a)
            dh = K.gemm_nt(da, shadow_swiglu(up_w, gate_w, transpose=True))
            dups = wgrad(da, h, [up_w, gate_w], swiglu_interleaved=True)
        else:
            dg_ = K.gemm_nt(dyd, shadow([down_w], transpose=True))
            if lora is not None and lora[2] is not None:
                dlora[2], dlora[3] = _lora_backward(dyd, g, lora[5], lora[2], lora[3], ctx.lora_scale, dg_)
            da = K.swiglu_bwd(a, dg_) if gated else K.gelu_bwd(a, dg_)
            dh = K.gemm_nt(da, shadow(ups, transpose=True))
            if lora is not None and lora[0] is not None:
                dlora[0], dlora[1] = _lora_backward(da, h, lora[4], lora[0], lora[1], ctx.lora_scale, dh)
            dups = wgrad(da, h, ups)
        dub = K.colsum(da) if has_ub else None
        if ctx.has_ln:
            dx, dgam, dbet = norm_bwd(dh, x2, ln_w, ctx.ln_b, mean, rstd, dres=dy2 if residual else None, kind=nkind)
        else:
            dx, dgam, dbet = (K.add(dh, dy2) if residual else dh), None, None
        return (dx.view(shp), dgam, dbet, dups[0], dub, dups[1] if gated else None, ddown, ddb, None), (None if lora is None else dlora)


class MlpBranchLora(torch.autograd.Function):
    """MlpBranch (the GELU MLP) with low-rank adapters on c_fc and / or c_proj (csrc/lora.hip); the base GEMMs, their routes and the
    frozen-parameter rules are MlpBranch's.  (A_up [r, d], B_up [hidden, r], A_down [r, hidden], B_down [d, r]), a pair may be None."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, up_w, up_b, gate_w, down_w, down_b, spec, scale, a_up, b_up, a_down, b_down):
        return MlpBranch.run_forward(ctx, x, ln_w, ln_b, up_w, up_b, gate_w, down_w, down_b, spec, (scale, a_up, b_up, a_down, b_down))

    @staticmethod
    def backward(ctx, dy):
        g, dl = MlpBranch.run_backward(ctx, dy)
        return (*g, None, *dl)


class NormLinear(torch.autograd.Function):
    """y = Linear([LN](x)) (+ bias);  heads (perceiver.ln_f -> to_motion / to_words, lm_head) and plain Linears."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w, b, eps, out_fp32):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        has_ln = ln_w is not None
        if has_ln:
            h, mean, rstd = K.norm_fwd(x2, ln_w.detach(), None if ln_b is None else ln_b.detach(), eps)
        else:
            h, mean, rstd = x2, None, None
        y = K.gemm_nt(h, shadow([w]), bias=None if b is None else shadow([b]),
                      out_dtype=torch.float32 if out_fp32 else None)
        ctx.has_ln, ctx.flags = has_ln, (ln_b is not None, b is not None)
        ctx.ln_b = ln_b
        ctx.save_for_backward(x, ln_w, w, h if has_ln else None, mean, rstd)
        return y.view(*shp[:-1], y.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        x, ln_w, w, h, mean, rstd = ctx.saved_tensors
        has_lnb, has_b = ctx.flags
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if h is None:
            h = x2
        dy2 = dy.contiguous().view(x2.shape[0], -1)
        if dy2.dtype != x2.dtype:
            dy2 = K.cast(dy2, x2.dtype)
        nout = dy2.shape[1]
        vec = 8 if dy2.dtype == torch.bfloat16 else 4
        npad = (nout + vec - 1) // vec * vec
        if npad != nout:   # e.g. vocab 50257: zero-pad the reduction dim of the dgrad / the rows of the wgrad operand
            dyp = torch.zeros((dy2.shape[0], npad), dtype=dy2.dtype, device=dy2.device)
            K.copy2d(dy2, dyp[:, :nout])
        else:
            dyp = dy2
        dh = K.gemm_nt(dyp, shadow([w], transpose=True, pad_n=npad))
        dw = K.gemm_tn(dyp, h)[:nout] if ctx.needs_input_grad[3] else None      # a frozen weight: no product
        db = K.colsum(dy2) if has_b and ctx.needs_input_grad[4] else None
        if ctx.has_ln:
            dx, dg, dbe = norm_bwd(dh, x2, ln_w, ctx.ln_b, mean, rstd)
        else:
            dx, dg, dbe = dh, None, None
        return dx.view(shp), dg, dbe, dw, db, None, None


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps, kind):
        y, mean, rstd = K.norm_fwd(x.contiguous(), w.detach(), None if b is None else b.detach(), eps, kind)
        ctx.kind, ctx.has_b, ctx.ln_b = kind, b is not None, b
        ctx.save_for_backward(x, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        dx, dg, db = norm_bwd(dy.contiguous(), x.contiguous(), w, ctx.ln_b, mean, rstd, kind=ctx.kind)
        return dx, dg, db, None, None


class PatchEmbed(torch.autograd.Function):
    """tokens = Linear(patch -> dim)(to_patches(x)) + space_embedding[c]  (models/brainformer.py:338-343).
    x is data (no gradient); K (= patch size) is zero-padded to a 16-byte multiple for the GEMM.  aug: an active AugmentConfig in a
    training forward (the caller has called augment_begin): the tokeniser launch draws the augmentation, one launch either way."""

    @staticmethod
    def forward(ctx, x, emb_w, emb_b, space, P, aug=None):
        B, T, Cn = x.shape
        d = emb_w.shape[0]
        dt = _COMPUTE_DTYPE
        kp = (P + 31) // 32 * 32
        xin = x if x.dtype == torch.float32 else K.cast(x.contiguous(), torch.float32)
        tok = K.patchify(xin.contiguous(), P, kp, dt) if aug is None else augment_tokens(xin, P, kp, dt, aug)
        sp = shadow([space.view(Cn, d)])
        h = K.gemm_nt(tok, shadow([emb_w], pad_k=kp), bias=shadow([emb_b]), residual=sp, res_rows=Cn)
        ctx.dims = (B, T // P, Cn, d, P)
        ctx.save_for_backward(tok)
        return h.view(B, (T // P) * Cn, d)

    @staticmethod
    def backward(ctx, dh):
        (tok,) = ctx.saved_tensors
        B, nT, Cn, d, P = ctx.dims
        dh2 = dh.contiguous().view(-1, d)
        dw = K.gemm_tn(dh2, tok)[:, :P].contiguous()
        db = K.colsum(dh2)
        dspace = K.colsum(dh2.view(B * nT, Cn * d)).view(1, Cn, d)
        return None, dw, db, dspace, None, None


def day_ids(date_info, B: int, device) -> Optional[Tensor]:
    """date_info as the kernels take it: None, or int64 [B] on `device`.  Accepts None, a Python int (broadcast over the batch) and an
    int64 / int32 tensor [B] on any device; the values are never read on the host."""
    if date_info is None:
        return None
    if isinstance(date_info, int):
        return torch.full((B,), date_info, dtype=torch.int64, device=device)
    if not isinstance(date_info, Tensor):
        date_info = torch.as_tensor(date_info)
    if date_info.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"date_info must be int64 or int32, got {date_info.dtype}")
    d = date_info.reshape(-1)
    if d.numel() != B:
        raise ValueError(f"date_info has {d.numel()} entries for a batch of {B}")
    return d.to(device=device, dtype=torch.int64).contiguous()


class DayPatchify(torch.autograd.Function):
    """tok [B, (T / P) * C, ldp] = to_patches(x + x @ delta[day] + bias[day]) in the compute dtype, columns P..ldp-1 zero
    (fk_day_adapter_fwd: the adapted signal never exists in memory).  x is data; day: int64 [B] on the device or None.  The backward
    takes d_tok in the same layout and returns (d_delta, d_bias) from fk_day_adapter_bwd; only x and day are saved.
    carrier=True returns (tok, carrier): autograd casts a gradient to the dtype of the tensor it belongs to, so an fp32 d_tok handed back
    for a bf16 tok would be rounded to bf16 on the way.  `carrier` is an fp32 tensor of tok's shape without memory (one element,
    expanded) whose only purpose is to own the fp32 gradient: PatchEmbedTok / MaskedPatchEmbedTok take it beside tok and return d_tok for
    it, unrounded.  out_fp32=True: tok itself in fp32 (the stand-alone P = 1 mode)."""

    @staticmethod
    def forward(ctx, x, day, delta, bias, P, ldp, out_fp32=False, carrier=False):
        B, T, Cn = x.shape
        xin = x if x.dtype == torch.float32 else K.cast(x.contiguous(), torch.float32)
        xin = xin.contiguous()
        tok = K.day_adapter_fwd(xin, day, delta.detach(), bias.detach(), P, ldp, torch.float32 if out_fp32 else _COMPUTE_DTYPE)
        ctx.P, ctx.dshape = P, tuple(delta.shape)
        ctx.save_for_backward(xin, day)
        ctx.set_materialize_grads(False)
        tok = tok.view(B, (T // P) * Cn, ldp)
        if not carrier:
            return tok
        return tok, torch.empty((1,), dtype=torch.float32, device=tok.device).expand(tok.shape)

    @staticmethod
    def backward(ctx, d_tok, d_carrier=None):
        x, day = ctx.saved_tensors
        g = d_carrier if d_carrier is not None else d_tok
        if g is None:
            return (None,) * 8
        d2 = g.contiguous().view(-1, g.shape[-1])
        if d2.dtype != torch.float32:
            d2 = K.cast(d2, torch.float32)
        d_delta, d_bias = K.day_adapter_bwd(x, day, d2, ctx.P, ctx.dshape)
        return None, None, d_delta, d_bias, None, None, None, None


def _d_tok(dh2: Tensor, emb_w: Tensor, kp: int) -> Tensor:
    """d_tok [rows, kp] fp32 = dh @ emb_w (columns P..kp-1 zero): the small-N NT GEMM on the transposed, K-padded weight shadow"""
    return K.gemm_nt(dh2, shadow([emb_w], transpose=True, pad_k=kp), out_dtype=torch.float32)


class PatchEmbedTok(torch.autograd.Function):
    """PatchEmbed on tokens that are a differentiable input (DayPatchify's): tok [B, nT * C, kp] compute dtype, kp = P rounded up to 32.
    The backward also returns d_tok = dh @ emb_w (fp32, same layout): for `carrier` (DayPatchify's, which keeps it fp32) when one is
    given, else for tok itself (autograd then casts it to tok's dtype)."""

    @staticmethod
    def forward(ctx, tok, emb_w, emb_b, space, P, carrier=None):
        B, N, kp = tok.shape
        Cn, d = space.shape[1], space.shape[2]
        tok2 = tok.view(B * N, kp)
        sp = shadow([space.view(Cn, d)])
        h = K.gemm_nt(tok2, shadow([emb_w], pad_k=kp), bias=shadow([emb_b]), residual=sp, res_rows=Cn)
        ctx.dims = (B, N // Cn, Cn, d, P, kp)
        ctx.save_for_backward(tok2, emb_w)
        return h.view(B, N, d)

    @staticmethod
    def backward(ctx, dh):
        tok2, emb_w = ctx.saved_tensors
        B, nT, Cn, d, P, kp = ctx.dims
        dh2 = dh.contiguous().view(-1, d)
        dw = K.gemm_tn(dh2, tok2)[:, :P].contiguous()
        db = K.colsum(dh2)
        dspace = K.colsum(dh2.view(B * nT, Cn * d)).view(1, Cn, d)
        to_carrier = ctx.needs_input_grad[5]
        d_tok = _d_tok(dh2, emb_w, kp).view(B, nT * Cn, kp) if (to_carrier or ctx.needs_input_grad[0]) else None
        return (None if to_carrier else d_tok), dw, db, dspace, None, (d_tok if to_carrier else None)


class ExpandQueries(torch.autograd.Function):
    """learnable_queries [1,M,d] (fp32 master) -> [B,M,d] compute dtype (models/brainformer.py:545)."""

    @staticmethod
    def forward(ctx, qparam, B):
        _, M, d = qparam.shape
        row = shadow([qparam.view(1, M * d)])
        out = torch.empty((B, M * d), dtype=row.dtype, device=row.device)
        K.copy2d(row.expand(B, M * d), out)
        ctx.shape = (M, d)
        return out.view(B, M, d)

    @staticmethod
    def backward(ctx, dy):
        M, d = ctx.shape
        return K.colsum(dy.contiguous().view(-1, M * d)).view(1, M, d), None


class L1Loss(torch.autograd.Function):
    """mean |d| (L1) or d^2 (MSE); optional per-row weights give the masked mean of SimpleMAE (models/simple_mae:393-395)."""

    @staticmethod
    def forward(ctx, pred, target, squared, row_weight=None):
        tgt = target if target.dtype == pred.dtype else K.cast(target.contiguous(), pred.dtype)
        p = pred.contiguous()
        loss2 = K.l1_loss_fwd(p, tgt.contiguous(), squared, row_weight)
        ctx.squared = squared
        ctx.save_for_backward(p, tgt.contiguous(), row_weight, loss2)
        return loss2[0]

    @staticmethod
    def backward(ctx, gout):
        p, tgt, row_weight, loss2 = ctx.saved_tensors
        g = gout.reshape(1).float().contiguous()
        return K.l1_loss_bwd(p, tgt, g, ctx.squared, row_weight, loss2), None, None, None


class CrossEntropy(torch.autograd.Function):
    """mean NLL over rows whose target != ignore_index; logits [rows, V] (any row stride)."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        loss2, lse = K.ce_loss_fwd(logits, targets.contiguous(), ignore_index)
        ctx.ignore = ignore_index
        ctx.save_for_backward(logits, targets, lse, loss2)
        return loss2[0]

    @staticmethod
    def backward(ctx, gout):
        logits, targets, lse, loss2 = ctx.saved_tensors
        g = gout.reshape(1).float().contiguous()
        d = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
        return K.ce_loss_bwd(logits, targets.contiguous(), lse, loss2, g, d, ctx.ignore), None, None


def cross_entropy(logits: Tensor, targets: Tensor, ignore_index: int = -100) -> Tensor:
    V = logits.shape[-1]
    lg = logits.reshape(-1, V) if logits.is_contiguous() else logits
    if lg.dim() != 2:
        lg = logits.contiguous().view(-1, V)
    return CrossEntropy.apply(lg, targets.reshape(-1), ignore_index)


class CTCLoss(torch.autograd.Function):
    """F.ctc_loss over logits [B, T, C] with the log-softmax folded in (csrc/ctc.hip): alpha and beta run side by side in the forward, the
    backward is one row-parallel launch.  'sum' / 'mean' return a scalar, 'none' the [B] losses.  Nothing here waits for the host."""

    @staticmethod
    def forward(ctx, logits, targets, input_lengths, target_lengths, blank, reduction, zero_infinity, pad_value):
        st = K.ctc_loss_fwd(logits, targets, input_lengths, target_lengths, blank, reduction, zero_infinity, pad_value,
                            want_grad=ctx.needs_input_grad[0])
        ctx.st = st
        ctx.save_for_backward(logits)
        return st.nll if reduction == "none" else st.loss2[0]

    @staticmethod
    def backward(ctx, gout):
        (logits,) = ctx.saved_tensors
        g = gout.reshape(-1).float().contiguous()
        return K.ctc_loss_bwd(logits, ctx.st, g), None, None, None, None, None, None, None


def ctc_loss(logits: Tensor, targets: Tensor, input_lengths: Optional[Tensor] = None, target_lengths: Optional[Tensor] = None, blank: int = 0,
             reduction: str = "mean", zero_infinity: bool = False, pad_value: int = -100) -> Tensor:
    """logits [B, T, C] (fp32 / bf16, batch first, NOT log-softmaxed), targets int64 [B, Lmax].  target_lengths None: a target ends at its
    first `pad_value` (the -100 label padding of utils.data_utils.pad_token_list), counted on the device; input_lengths None: T frames
    each.  Up to 255 labels per target."""
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    if targets.dim() == 2 and targets.shape[1] > 0 and targets.stride(1) != 1:
        targets = targets.contiguous()
    return CTCLoss.apply(logits, targets, input_lengths, target_lengths, blank, reduction, zero_infinity, pad_value)


@torch.no_grad()
def ctc_greedy_decode(logits: Tensor, input_lengths: Optional[Tensor] = None, blank: int = 0, pad: int = -100):
    """Best-path decoding: per-frame argmax, repeats merged, blanks dropped -> (ids int64 [B, T] padded with `pad`, lengths int64 [B])."""
    B, T, Cn = logits.shape
    lg = logits.reshape(B * T, Cn) if logits.is_contiguous() else logits.contiguous().view(B * T, Cn)
    return K.ctc_collapse(K.argmax_rows(lg).view(B, T), input_lengths, blank, pad)


@torch.no_grad()
def ctc_beam_decode(logits: Tensor, input_lengths: Optional[Tensor] = None, blank: int = 0, beam_width: int = 8, topk: Optional[int] = None,
                    nbest: int = 1, pad: int = -100):
    """Prefix beam search: the nbest most probable LABELLINGS (the best path is the most probable alignment) -> (ids int64 [B, nbest, T]
    padded with `pad`, lengths int64 [B, nbest], scores fp32 [B, nbest], best first).  Logits fp32 or bf16 as the model gives them; two
    launches, nothing waits for the host.  The n-best list with its scores is what a language model rescores."""
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    return K.ctc_beam_search(logits, input_lengths, blank, beam_width, topk, nbest, pad)


@torch.no_grad()
def ctc_beam_decode_lm(logits: Tensor, lm, input_lengths: Optional[Tensor] = None, blank: int = 0, beam_width: int = 8, topk: Optional[int] = None,
                       nbest: int = 1, lm_weight: float = 1.0, length_bonus: float = 0.0, use_eos: bool = True, pad: int = -100):
    """Prefix beam search with n-gram shallow fusion: the backoff model `lm` (utils.ngram.NGramLM over the head's classes) takes part in
    every selection, so a labelling the acoustic model alone would have dropped can stay in the beam, which no rescoring of the final
    list can do.  The beam is ranked by CTC total + lm_weight * ln P_lm(labelling) + length_bonus * length, at the end (use_eos) + lm_weight
    * ln P_lm(</s> | labelling) -> (ids int64 [B, nbest, T] padded with `pad`, lengths int64 [B, nbest], am fp32 [B, nbest] the pure CTC
    score, lm fp32 [B, nbest] the unweighted ln P_lm, total fp32 [B, nbest] the ranking key), best first.  Two launches, nothing waits for
    the host; the model's tables are copied to the device once."""
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    return K.ctc_beam_search_lm(logits, lm, input_lengths, blank, beam_width, topk, nbest, lm_weight, length_bonus, use_eos, pad)


class CtcLexiconResult(NamedTuple):
    """engine.ctc_beam_decode_lexicon's result, best first.  words int64 [B, nbest, (T + 1) // 2] padded with `pad`, word_lengths int64
    [B, nbest]; ids int64 [B, nbest, T] / lengths: the labelling (separators included); am (the CTC mass), lm (the unweighted ln P of the
    word model), total (the ranking key) fp32 [B, nbest]; complete uint8 [B, nbest]: the labelling ends at a word boundary."""
    words: Tensor
    word_lengths: Tensor
    ids: Tensor
    lengths: Tensor
    am: Tensor
    lm: Tensor
    total: Tensor
    complete: Tensor


@torch.no_grad()
def ctc_beam_decode_lexicon(logits: Tensor, lexicon, lm=None, sep: int = 1, input_lengths: Optional[Tensor] = None, blank: int = 0,
                            beam_width: int = 8, topk: Optional[int] = None, nbest: int = 1, lm_weight: float = 1.0, word_bonus: float = 0.0,
                            use_eos: bool = True, pad: int = -100) -> CtcLexiconResult:
    """Prefix beam search over a phoneme / letter head that returns WORDS: the search is constrained to labellings that spell words of
    `lexicon` (utils.lexicon.Lexicon) separated by the class `sep`; at every word end the word-level backoff model `lm` (utils.ngram.NGramLM
    over the lexicon's word ids, None: none) picks among homophones and adds lm_weight * ln P_lm(word | words so far) + word_bonus to the
    ranking key, at the end (use_eos) lm_weight * ln P_lm(</s>).  A hypothesis whose last word is finished (with or without a final sep) is
    complete and ranks before every incomplete one.  Two launches, nothing waits for the host; the tables are copied to the device once.
    Not built: LM look-ahead into the trie, an unknown-word path, forking on homophones (one word per labelling, chosen greedily)."""
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    return CtcLexiconResult(*K.ctc_beam_search_lex(logits, lexicon, lm, sep, input_lengths, blank, beam_width, topk, nbest, lm_weight, word_bonus,
                                                   use_eos, pad))


class CtcAlignment(NamedTuple):
    """engine.ctc_forced_align's result.  score fp32 [B]: the log-probability of the best alignment (-inf: the sample has none); path int64
    [B, T]: the class per frame (`pad` behind the sample's end); index int64 [B, T]: the label of the target a frame emits (-1: blank or
    behind the end); start / end int64 [B, Lmax]: label i holds the frames [start, end) (-1 / -1 behind the target's end); label_lp fp32
    [B, Lmax]: the sum of the label's frame log-probabilities."""
    score: Tensor
    path: Tensor
    index: Tensor
    start: Tensor
    end: Tensor
    label_lp: Tensor

    @property
    def confidence(self) -> Tensor:
        """fp32 [B, Lmax]: exp(label_lp / (end - start)), the geometric mean of the posteriors of the label's class over its frames; 0 where
        there is no label"""
        n = (self.end - self.start).clamp(min=1).to(torch.float32)
        return torch.where(self.end > self.start, torch.exp(self.label_lp / n), torch.zeros_like(self.label_lp))


@torch.no_grad()
def ctc_forced_align(logits: Tensor, targets: Tensor, input_lengths: Optional[Tensor] = None, target_lengths: Optional[Tensor] = None,
                     blank: int = 0, pad_value: int = -100, pad: int = -100) -> CtcAlignment:
    """Forced alignment: the most probable alignment of logits [B, T, C] (fp32 / bf16, batch first, NOT log-softmaxed) to targets int64
    [B, Lmax] (Viterbi over the CTC lattice; exact ties and corner cases: include/franken_hip.h, fk_ctc_align).  Lengths as ctc_loss:
    target_lengths None: a target ends at its first `pad_value`; input_lengths None: T frames each; up to 255 labels.  The result is
    indices and detached floats: no autograd graph.  Two launches, nothing waits for the host."""
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    if targets.dim() == 2 and targets.shape[1] > 0 and targets.stride(1) != 1:
        targets = targets.contiguous()
    r = K.ctc_align(logits.detach(), targets, input_lengths, target_lengths, blank, pad_value, pad)
    return CtcAlignment(r["score"], r["path"], r["index"], r["start"], r["end"], r["label_lp"])


# ---- edit distance on the device (csrc/editdist.hip): error rates, the oracle error of a list, MBR re-ranking and the MWER loss ----

def _seq3(t: Tensor, lens: Optional[Tensor], pad_value: int):
    """[B, L] or [B, n, L] ids (+ lengths [B] / [B, n]) -> int64 [B, n, L] with unit token stride and L >= 1, lengths int64 [B, n] or None"""
    assert t.dtype == torch.int64 and t.dim() in (2, 3), "ids: int64 [B, L] or [B, n, L]"
    if t.dim() == 2:
        t = t.unsqueeze(1)
    if lens is not None:
        lens = lens.to(torch.int64).reshape(t.shape[0], t.shape[1]).contiguous()
    if t.shape[2] == 0:                                   # a column-less array holds empty sequences
        t = t.new_full((t.shape[0], t.shape[1], 1), pad_value)
    elif t.stride(2) != 1:
        t = t.contiguous()
    return t, lens


@torch.no_grad()
def edit_distance(a: Tensor, b: Tensor, a_lengths: Optional[Tensor] = None, b_lengths: Optional[Tensor] = None, pad_value: int = -100) -> Tensor:
    """Unit-cost Levenshtein distances on int64 ids, on the device (the host yardstick is utils.metrics.edit_distance).  a [P, La] against
    b [P, Lb] -> int32 [P] (pair by pair); a [B, La] against b [B, n, Lb] -> int32 [B, n] (a sentence's reference against its n
    hypotheses); a [B, n, La] against b [B, n, Lb] -> int32 [B, n].  Lengths int64 of the leading shape, or None: a sequence ends at its
    first `pad_value` (the -100 label padding).  At most 1024 tokens per row and 32 sequences per group.  One launch, nothing waits for the
    host."""
    flat = b.dim() == 2
    a3, al = _seq3(a, a_lengths, pad_value)
    b3, bl = _seq3(b, b_lengths, pad_value)
    d = K.edit_distance(a3, al, b3, bl, pad_value)
    return d[:, 0] if flat else d


@torch.no_grad()
def error_rate(references: Tensor, hypotheses: Tensor, reference_lengths: Optional[Tensor] = None, hypothesis_lengths: Optional[Tensor] = None,
               pad_value: int = -100):
    """The corpus error rate of utils.metrics.token_error_rate without leaving the device: references int64 [B, Lr], hypotheses int64
    [B, Lh] (lengths int64 [B], or None: -100 padded) -> (rate, errors, ref_lengths): rate the fp32 device scalar sum(errors) /
    sum(reference lengths) (nan for an empty corpus of references), errors int32 [B], ref_lengths int32 [B].  No synchronisation: read
    rate with .item() when the number is wanted."""
    assert references.dim() == 2 and hypotheses.dim() == 2
    a3, al = _seq3(references, reference_lengths, pad_value)
    b3, bl = _seq3(hypotheses, hypothesis_lengths, pad_value)
    d, alen = K.edit_distance(a3, al, b3, bl, pad_value, want_lengths=True)
    errors, ref_lengths = d[:, 0], alen[:, 0]
    return errors.sum().to(torch.float32) / ref_lengths.sum().to(torch.float32), errors, ref_lengths


@torch.no_grad()
def nbest_oracle(ids: Tensor, lengths: Tensor, scores: Optional[Tensor], targets: Tensor, target_lengths: Optional[Tensor] = None,
                 pad_value: int = -100):
    """The oracle error of an n-best list (is the beam wide enough?): ids int64 [B, n, T], lengths int64 [B, n], scores fp32 [B, n] or
    None, targets int64 [B, L] -> (errors int32 [B], index int64 [B]): the smallest distance to the reference over the valid hypotheses
    (finite score) and the first hypothesis that has it; a sentence without a valid hypothesis: 2^31 - 1 and index 0."""
    a3, al = _seq3(targets, target_lengths, pad_value)
    b3, bl = _seq3(ids, lengths, pad_value)
    d = K.edit_distance(a3, al, b3, bl, pad_value)
    if scores is not None:
        d = torch.where(torch.isfinite(scores), d, torch.full_like(d, 2 ** 31 - 1))
    best, index = d.min(dim=1)
    first = (d == best[:, None]).to(torch.int64).argmax(dim=1)          # min's index among equals is unspecified; the first one is wanted
    return best, first


class MbrResult(NamedTuple):
    """engine.mbr_rerank's result, best (smallest expected distance) first: ids int64 [B, n, T] padded with `pad`, lengths int64 [B, n],
    scores fp32 [B, n] (the input scores in the new order), risk fp32 [B, n] (+inf for an invalid hypothesis), order int64 [B, n] (the
    input index of each place), n_valid int64 [B], dist int32 [B, n, n] in INPUT order (-1 in an invalid hypothesis' row and column)."""
    ids: Tensor
    lengths: Tensor
    scores: Tensor
    risk: Tensor
    order: Tensor
    n_valid: Tensor
    dist: Tensor


@torch.no_grad()
def mbr_rerank(ids: Tensor, lengths: Tensor, scores: Tensor, scale: float = 1.0, pad: int = -100) -> MbrResult:
    """Minimum-Bayes-risk selection from n-best lists (ids int64 [B, n, T], lengths int64 [B, n], scores fp32 [B, n]: what
    ctc_beam_decode, ctc_beam_decode_lm or GPT.rescore_nbest return): under the posterior softmax(scale * scores) over a sentence's valid
    hypotheses (finite score) every hypothesis gets its EXPECTED edit distance to the others, and the list comes back by ascending risk;
    exact ties go to the better-scored (earlier) hypothesis, invalid ones last.  scale = 0 is the uniform posterior (the list's medoid), a
    large scale returns the best-scored hypothesis.  Two launches, nothing waits for the host."""
    if ids.stride(-1) != 1:
        ids = ids.contiguous()
    lengths, scores = lengths.contiguous(), scores.to(torch.float32).contiguous()
    dist = K.nbest_pairwise_distance(ids, lengths, scores)
    _, (o_ids, o_len, o_sc, o_risk, order, n_valid) = K.mbr_rank(dist, ids, lengths, scores, scale, pad)
    return MbrResult(o_ids, o_len, o_sc, o_risk, order, n_valid, dist)


class CtcMwerLoss(torch.autograd.Function):
    """mwer_weight * MWER + ce_weight * CTC as ONE node over the logits: the forward is the CTC lattice of every hypothesis on the logits
    expanded n times (reduction none), fk_mwer_combine and, with ce_weight, the CTC loss of the targets; the backward is kernel launches and
    pointwise scaling only (the CTC backward of the expanded rows scaled by grad_out * coef / count, fk_mwer_reduce_rows back to [B, T, C]
    on top of the CTC term's gradient), so one gradient reaches the logits and no reduction or accumulation is left to the autograd
    engine inside a captured step.  A row the combine ruled out is never read: its CTC backward is NaN whatever it is scaled by."""

    @staticmethod
    def forward(ctx, logits, targets, input_lengths, target_lengths, hyp_targets, hyp_frames, hyp_lengths, errors, scores, lengths, blank,
                mwer_weight, ce_weight, zero_infinity, pad_value):
        B, T, Cn = logits.shape
        n = errors.shape[1]
        want = ctx.needs_input_grad[0]
        lx = logits.detach().unsqueeze(1).expand(B, n, T, Cn).reshape(B * n, T, Cn)
        st = K.ctc_loss_fwd(lx, hyp_targets, hyp_frames, hyp_lengths, blank, "none", False, pad_value, want_grad=want)
        loss_b, coef, count, valid = K.mwer_combine(st.nll.view(B, n), errors, scores, lengths, 255)
        count = count.clamp(min=1.0)
        loss = loss_b.sum() / count[0]
        if mwer_weight != 1.0:
            loss = mwer_weight * loss
        st_ce = None
        if ce_weight:
            st_ce = K.ctc_loss_fwd(logits.detach(), targets, input_lengths, target_lengths, blank, "mean", zero_infinity, pad_value,
                                    want_grad=want)
            loss = loss + ce_weight * st_ce.loss2[0]
        ctx.st, ctx.st_ce, ctx.weights = st, st_ce, (mwer_weight, ce_weight)
        ctx.save_for_backward(logits, lx, coef, count, valid)
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, lx, coef, count, valid = ctx.saved_tensors
        mwer_weight, ce_weight = ctx.weights
        g = gout.reshape(()).float()
        dlogits = None
        if ctx.st_ce is not None:
            dlogits = K.ctc_loss_bwd(logits, ctx.st_ce, (g * ce_weight).reshape(1).contiguous())
            if not dlogits.is_contiguous():
                dlogits = dlogits.contiguous()
        rows = K.ctc_loss_bwd(lx, ctx.st, ((g * mwer_weight) * coef / count[0]).reshape(-1).contiguous())
        dlogits = K.mwer_reduce_rows(rows, valid, dlogits, accumulate=dlogits is not None)
        return (dlogits,) + (None,) * 14


def ctc_mwer_loss(logits: Tensor, targets: Tensor, beam_width: int = 8, nbest: int = 4, topk: Optional[int] = None, blank: int = 0,
                  ce_weight: float = 0.0, hyps=None, input_lengths: Optional[Tensor] = None, target_lengths: Optional[Tensor] = None,
                  pad_value: int = -100, mwer_weight: float = 1.0, zero_infinity: bool = False) -> Tensor:
    """Minimum-word-error-rate loss of a CTC head: over the n-best list of each sentence, sum_i p_i (errors_i - mean errors) with p =
    softmax(-nll) renormalised over the list, averaged over the sentences; the result is mwer_weight * that + ce_weight * ctc_loss(logits,
    targets) (reduction 'mean', with this zero_infinity).  It trains the head on the metric itself.  logits [B, T, C] (fp32 / bf16, NOT log-softmaxed), targets int64
    [B, Lmax] as ctc_loss takes them.

    The list is ctc_beam_decode(beam_width, topk, nbest) on the detached logits, or the caller's hyps = (ids int64 [B, n, Th], lengths
    int64 [B, n], scores fp32 [B, n]).  nll[b, i] is the exact full-sum CTC loss of hypothesis i (the CTC lattice kernels, reduction 'none',
    NOT the pruned beam score), errors[b, i] its edit distance to the target (engine.edit_distance), and the gradient flows through nll
    only.  A hypothesis is left out when its beam score or its nll is not finite (an empty beam slot, an infeasible labelling) or when it
    has more than 255 labels (the CTC envelope); a sentence without a hypothesis contributes 0.  With nbest = 1 the loss and its gradient
    are 0.

    Cost: the logits are expanded to [B * n, T, C], so the step holds n copies of the logits and of their gradient: nothing for a 41-class
    phoneme head, about 1.6 GB of fp32 gradient at B = 32, n = 8, 32 x 50258.  Nothing waits for the host (graph-capturable); the whole
    loss is one autograd node (CtcMwerLoss), so one gradient reaches the logits."""
    assert logits.dim() == 3 and targets.dim() == 2 and targets.dtype == torch.int64
    B, T, Cn = logits.shape
    if logits.stride(-1) != 1 or not logits.is_contiguous():
        logits = logits.contiguous()
    if targets.shape[1] > 0 and targets.stride(1) != 1:
        targets = targets.contiguous()
    with torch.no_grad():
        if hyps is None:
            ids, lengths, scores = ctc_beam_decode(logits.detach(), input_lengths, blank, beam_width, topk, nbest, pad_value)
        else:
            ids, lengths, scores = hyps
        n, Th = ids.shape[1], ids.shape[2]
        errors = edit_distance(targets, ids, target_lengths, lengths, pad_value)
        W = min(Th, 255)                                  # the host decides by the column count; a longer hypothesis is left out by its length
        hyp_targets = ids[:, :, :W].reshape(B * n, W)
        hyp_lengths = lengths.clamp(0, W).reshape(B * n)
        hyp_frames = None if input_lengths is None else input_lengths.repeat_interleave(n, output_size=B * n)
        scores = scores.to(torch.float32).contiguous()
        lengths = lengths.contiguous() if Th > 255 else None
    return CtcMwerLoss.apply(logits, targets, input_lengths, target_lengths, hyp_targets, hyp_frames, hyp_lengths, errors, scores, lengths, blank,
                             float(mwer_weight), float(ce_weight), bool(zero_infinity), pad_value)


class HeadCrossEntropy(torch.autograd.Function):
    """loss = mean CE(Linear([LN](x)), targets) over the rows whose target != ignore_index, WITHOUT a [rows, V] tensor in either
    direction: lm_head + F.cross_entropy of models/gpt2_model.py:205-210 and the `to_words` head of the notebook CE BrainFormer, used when
    the caller does not need the logits (`fuse_head_loss`).
    forward : ONE product — fk_head_ce_fwd keeps every 128 x 128 logits tile in the MFMA accumulators and emits per-row (max, sum exp,
              target logit); fk_ce_chunk_finish turns them into the row log-sum-exp and the loss.
    backward: the product again with the vocabulary on the lane, its epilogue writing the TRANSPOSED d-logits dlT [V, rows] (bf16 in the
              throughput mode: 80 MB at rows = 800, V = 50257), so that dH = dlT^T W is a contraction over the vocabulary (fk_gemm_tn, split
              slabs) and dW = dlT H (fk_gemm_nt over the rows) — no GEMM with K = 50257 and 21 workgroups.
    Targets outside [0, V) other than ignore_index contribute nothing to the loss' numerator but count as valid rows in neither
    (F.cross_entropy would raise): callers pass token ids.  `chunk` is accepted for compatibility and unused."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w, b, targets, eps, ignore_index, chunk):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        V = w.shape[0]
        has_ln = ln_w is not None
        if has_ln:
            h, mean, rstd = K.norm_fwd(x2, ln_w.detach(), None if ln_b is None else ln_b.detach(), eps)
        else:
            h, mean, rstd = to_compute(x2), None, None
        vec = 8 if h.dtype == torch.bfloat16 else 4
        npad = (V + vec - 1) // vec * vec
        wsh = shadow([w], pad_n=npad)
        bsh = None if b is None else shadow([b])
        tg = targets.reshape(-1).contiguous()
        loss2, lse = K.head_ce_fwd(h, wsh, bsh, tg, V, ignore_index)
        ctx.cfg = (has_ln, b is not None, ignore_index, npad)
        ctx.ln_b = ln_b
        ctx.save_for_backward(x, ln_w, w, b, h, mean, rstd, tg, lse, loss2)
        return loss2[0]

    @staticmethod
    def backward(ctx, gout):
        x, ln_w, w, b, h, mean, rstd, tg, lse, loss2 = ctx.saved_tensors
        has_ln, has_b, ignore_index, npad = ctx.cfg
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        rows, d, V = h.shape[0], h.shape[1], w.shape[0]
        g = gout.reshape(1).float().contiguous()
        wsh = shadow([w], pad_n=npad)
        bsh = shadow([b]) if has_b else None
        rows_pad = (rows + 63) // 64 * 64                                   # K of the weight-gradient product: whole 64-element k-tiles
        dlT, db = K.head_ce_bwd(h, wsh, bsh, tg, lse, loss2, g, V, npad, rows_pad, has_b, ignore_index)
        dh32 = K.gemm_tn(dlT, wsh)                                          # [rows_pad, d] = sum_v dlT[v, m] W[v, :]
        dh = dh32[:rows] if h.dtype == torch.float32 else K.cast(dh32[:rows], h.dtype)
        dw = None
        if ctx.needs_input_grad[3]:                                         # a frozen head: neither the transpose nor the [V, d] product
            hT = torch.zeros((d, rows_pad), dtype=h.dtype, device=h.device)
            K.transpose2d(h, out=hT)
            dw = K.gemm_nt(dlT, hT, out_dtype=torch.float32)[:V]            # [V, d] = sum_m dlT[v, m] H[m, :]
        if has_ln:
            dx, dg, dbe = norm_bwd(dh, x2, ln_w, ctx.ln_b, mean, rstd)
        else:
            dx, dg, dbe = (dh if dh.dtype == x2.dtype else K.cast(dh, x2.dtype)), None, None
        return dx.view(shp), dg, dbe, dw, db, None, None, None, None


def head_cross_entropy(x: Tensor, ln_w, ln_b, w: Tensor, b, targets: Tensor, eps: float = 1e-5, ignore_index: int = -100,
                       chunk: int = 8192) -> Tensor:
    return HeadCrossEntropy.apply(x, ln_w, ln_b, w, b, targets, eps, ignore_index, chunk)


def l1_loss(pred: Tensor, target: Tensor) -> Tensor:
    return L1Loss.apply(pred, target, False)


def mse_loss(pred: Tensor, target: Tensor, row_weight: Optional[Tensor] = None) -> Tensor:
    return L1Loss.apply(pred, target, True, row_weight)


# --------------------------------------------------------------------------------------------- conv stack
def _conv_shadow(w: Tensor, mode: str, transpose: bool) -> Tensor:
    """GEMM-shaped compute-dtype view of a convolution weight (re-packed lazily when the master changes):
    mode "conv":  nn.Conv1d weight [Cout, Cin, K]          -> W' [Cout, K*Cin],   W'[o, k*Cin + c] = W[o, c, k]
    mode "convT": nn.ConvTranspose1d weight [Cin, Cout, 2s] -> W' [s*Cout, 2*Cin], row (r, o), taps (x[j-1], x[j]):
                  W'[(r,o), c] = W[c, o, r + s],  W'[(r,o), Cin + c] = W[c, o, r]      (models/vq_brain.py:31-45)."""
    key = (("conv", mode, w.data_ptr(), tuple(w.shape)), transpose, _COMPUTE_DTYPE)
    ent = _shadow_entry(key, (w,))
    stamp = ent.current_stamp()
    if ent.stamp == stamp:
        return ent.tensor
    wref = ent.params[0]

    def pack():
        wd = wref().detach()
        if mode == "conv":
            g = wd.permute(0, 2, 1).reshape(wd.shape[0], -1)
        else:
            cin, cout, k2 = wd.shape
            s_ = k2 // 2
            g = torch.cat([wd[:, :, s_:].permute(2, 1, 0), wd[:, :, :s_].permute(2, 1, 0)], dim=2).reshape(s_ * cout, 2 * cin)
        g = g.t() if transpose else g
        if ent.tensor is None:
            ent.tensor = torch.empty(g.shape, dtype=_COMPUTE_DTYPE, device=wd.device)
        ent.tensor.copy_(g)                 # in place: the storage a captured GEMM reads stays the same across optimizer steps

    ent.repack = pack
    pack()
    ent.stamp = stamp
    return ent.tensor


def _conv_wgrad_to_master(dwp: Tensor, w: Tensor, mode: str) -> Tensor:
    """inverse of the _conv_shadow layout for the fp32 weight gradient"""
    if mode == "conv":
        cout, cin, k = w.shape
        return dwp.view(cout, k, cin).permute(0, 2, 1).contiguous()
    cin, cout, k2 = w.shape
    s_ = k2 // 2
    t = dwp.view(s_, cout, 2, cin)                       # [r, o, tap, c]
    return torch.cat([t[:, :, 1].permute(2, 1, 0), t[:, :, 0].permute(2, 1, 0)], dim=2).contiguous()   # [c, o, (r | r + s)]


class CausalConv1dFn(torch.autograd.Function):
    """Channels-last causal convolution as im2col + MFMA GEMM (bias and an optional residual fused in the GEMM epilogue).
    mode "conv": y[b, t, :] = sum_k W[:, :, k] x[b, t*stride + k*dil - dil*(K-1), :] + bias  (CausalConv1d, models/vq_brain.py:22-28)
    mode "convT": CausalConvTranspose1d(kernel 2s, stride s): [B, T, Cin] -> [B, s*T, Cout]  (:31-45)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, dil, mode, residual):
        B, T, cin = x.shape
        if mode == "conv":
            cout, _, ks = w.shape
            st, n_rep = stride, 1
        else:
            _, cout, k2 = w.shape
            ks, st, n_rep = 2, 1, k2 // 2
            assert k2 == 2 * stride and dil == 1, "CausalConvTranspose1d is built for kernel_size = 2 * stride"
        x = x.contiguous()
        cols = x.view(B * T, cin) if (ks == 1 and st == 1) else K.im2col1d(x, ks, st, dil)
        bias = None
        if b is not None:
            bias = shadow([b]) if n_rep == 1 else K.cast(b.detach().repeat(n_rep), _COMPUTE_DTYPE)
        res2 = None if residual is None else residual.contiguous().view(cols.shape[0], -1)
        y = K.gemm_nt(cols, _conv_shadow(w, mode, False), bias, residual=res2)
        tout = (T - 1) // st + 1
        ctx.cfg = (B, T, cin, ks, st, dil, mode, n_rep, b is not None, residual is not None)
        ctx.save_for_backward(x, w)
        return y.view(B, tout * n_rep, cout)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, T, cin, ks, st, dil, mode, n_rep, has_b, has_res = ctx.cfg
        dy = dy.contiguous()
        dy2 = dy.view(-1, dy.shape[-1] * n_rep)
        cols = x.view(B * T, cin) if (ks == 1 and st == 1) else K.im2col1d(x, ks, st, dil)
        dcols = K.gemm_nt(dy2, _conv_shadow(w, mode, True))
        dx = dcols.view(B, T, cin) if (ks == 1 and st == 1) else K.col2im1d(dcols, B, T, cin, ks, st, dil)
        dw = _conv_wgrad_to_master(K.gemm_tn(dy2, cols), w, mode)
        db = None
        if has_b:
            db = K.colsum(dy2)
            if n_rep > 1:
                db = db.view(n_rep, -1).sum(0)
        return dx, dw, db, None, None, None, (dy if has_res else None)


class EluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return K.elu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return K.elu_bwd(x, dy.contiguous())


class StraightThrough(torch.autograd.Function):
    """forward: the quantized vectors; backward: the gradient goes to the encoder output unchanged (x + (q - x).detach())."""

    @staticmethod
    def forward(ctx, x, q):
        return q

    @staticmethod
    def backward(ctx, dq):
        return dq, None


class VQLookupFn(torch.autograd.Function):
    """(x [..., D], codes fp32 [K, D], commitment_weight) -> (q, idx, commit): the nearest unit-norm code of every row in one launch
    (fk_vq_assign: exact fp32 cosine similarity for either compute dtype, lowest index on a tie), q = codes[idx] in x's dtype as the
    straight-through output, idx int64 [...], commit = commitment_weight * mean((x - q)^2) as an fp32 scalar.  counts [K] / sums [K, D]
    (K.vq_stats) collect the per-code row counts and unit-norm row sums of the same launch.  Backward: dx = dq + dcommit * 2 *
    commitment_weight / numel * (x - q) in one launch (fk_vq_bwd); no gradient goes to the codes."""

    @staticmethod
    def forward(ctx, x, codes, commitment_weight, counts=None, sums=None):
        D = x.shape[-1]
        x2 = x.detach().reshape(-1, D)
        if x2.stride(1) != 1 or x2.stride(0) % 4 != 0:
            x2 = x2.contiguous()
        idx, q, commit = K.vq_assign(x2, codes.detach(), True, counts, sums, commitment_weight / x2.numel())
        ctx.save_for_backward(x2, q)
        ctx.c_scale = 2.0 * commitment_weight / x2.numel()
        ctx.xshape = x.shape
        idx = idx.view(x.shape[:-1])
        ctx.mark_non_differentiable(idx)
        return q.view(x.shape), idx, commit.view(())

    @staticmethod
    def backward(ctx, dq, _didx, dcommit):
        x2, q = ctx.saved_tensors
        if dq is not None:
            dq = dq.reshape(x2.shape).contiguous()
        if dcommit is not None:
            dcommit = dcommit.reshape(1).float().contiguous()
        dx = K.vq_bwd(x2.contiguous(), q, dq, dcommit, ctx.c_scale)
        return dx.view(ctx.xshape), None, None, None, None


# --------------------------------------------------------------------------------------------- MAE pieces
class GatherRows(torch.autograd.Function):
    """out[b, i, :] = src[b, idx[b, i], :]  (models/brainformer.py:441,468); idx rows are unique per sample."""

    @staticmethod
    def forward(ctx, src, idx):
        ctx.n_src = src.shape[1]
        ctx.save_for_backward(idx)
        return K.gather_rows(src.contiguous(), idx)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dy = dy.contiguous()
        d = torch.zeros((dy.shape[0], ctx.n_src, dy.shape[2]), dtype=dy.dtype, device=dy.device)
        K.scatter_rows_(d, idx, dy)
        return d, None


class MaskedPatchEmbed(torch.autograd.Function):
    """tokens = emb(patches[b, unmasked]) + spatial_pos_embedding[b, unmasked]  (models/brainformer.py:429-444)."""

    @staticmethod
    def forward(ctx, tok_all, emb_w, emb_b, space, unmasked, P):
        B, N, kp = tok_all.shape
        Cn, d = space.shape[1], space.shape[2]
        tok_u = K.gather_rows(tok_all, unmasked)                                   # [B, n, kp]
        sp = K.gather_rows(shadow([space.view(Cn, d)]), unmasked, idx_mod=Cn)     # spatial rows repeat every Cn tokens
        n = unmasked.shape[1]
        h = K.gemm_nt(tok_u.view(B * n, kp), shadow([emb_w], pad_k=kp), bias=shadow([emb_b]), residual=sp.view(B * n, d))
        ctx.dims = (B, n, Cn, d, P)
        ctx.save_for_backward(tok_u, unmasked)
        return h.view(B, n, d)

    @staticmethod
    def backward(ctx, dh):
        tok_u, unmasked = ctx.saved_tensors
        B, n, Cn, d, P = ctx.dims
        dh2 = dh.contiguous().view(B * n, d)
        dw = K.gemm_tn(dh2, tok_u.view(B * n, -1))[:, :P].contiguous()
        db = K.colsum(dh2)
        dspace = torch.zeros((Cn, d), dtype=torch.float32, device=dh.device)
        K.scatter_add_rows_(dspace, unmasked, dh2, idx_mod=Cn)
        return None, dw, db, dspace.view(1, Cn, d), None, None


class MaskedPatchEmbedTok(torch.autograd.Function):
    """MaskedPatchEmbed on tokens that are a differentiable input (DayPatchify's): the backward also returns d_tok_all, dh @ emb_w of the
    kept tokens scattered into a zeroed [B, n_tokens, kp] (fp32), for `carrier` when one is given (see PatchEmbedTok)."""

    @staticmethod
    def forward(ctx, tok_all, emb_w, emb_b, space, unmasked, P, carrier=None):
        B, N, kp = tok_all.shape
        Cn, d = space.shape[1], space.shape[2]
        tok_u = K.gather_rows(tok_all, unmasked)
        sp = K.gather_rows(shadow([space.view(Cn, d)]), unmasked, idx_mod=Cn)
        n = unmasked.shape[1]
        h = K.gemm_nt(tok_u.view(B * n, kp), shadow([emb_w], pad_k=kp), bias=shadow([emb_b]), residual=sp.view(B * n, d))
        ctx.dims = (B, n, N, Cn, d, P, kp)
        ctx.save_for_backward(tok_u, unmasked, emb_w)
        return h.view(B, n, d)

    @staticmethod
    def backward(ctx, dh):
        tok_u, unmasked, emb_w = ctx.saved_tensors
        B, n, N, Cn, d, P, kp = ctx.dims
        dh2 = dh.contiguous().view(B * n, d)
        dw = K.gemm_tn(dh2, tok_u.view(B * n, -1))[:, :P].contiguous()
        db = K.colsum(dh2)
        dspace = torch.zeros((Cn, d), dtype=torch.float32, device=dh.device)
        K.scatter_add_rows_(dspace, unmasked, dh2, idx_mod=Cn)
        d_tok, to_carrier = None, ctx.needs_input_grad[6]
        if to_carrier or ctx.needs_input_grad[0]:
            d_tok = torch.zeros((B, N, kp), dtype=torch.float32, device=dh.device)
            K.scatter_rows_(d_tok, unmasked, _d_tok(dh2, emb_w, kp).view(B, n, kp))
        return (None if to_carrier else d_tok), dw, db, dspace.view(1, Cn, d), None, None, (d_tok if to_carrier else None)


class AssembleDecoder(torch.autograd.Function):
    """dec[b, unmasked] = tokens, dec[b, masked] = mask_token, + decoder_pos_emb[cat(unmasked, masked)] added in
    CONCATENATION order (the reference's quirk, models/brainformer.py:455-460)."""

    @staticmethod
    def forward(ctx, tokens, mask_token, pos_table, unmasked, masked):
        B, n, dd = tokens.shape
        N = n + masked.shape[1]
        row = shadow([mask_token.view(1, dd)])
        dec = torch.empty((B, N, dd), dtype=tokens.dtype, device=tokens.device)
        K.copy2d(row.expand(B * N, dd), dec.view(B * N, dd))                       # every row = mask_token ...
        K.scatter_rows_(dec, unmasked, tokens.contiguous())                        # ... then the visible tokens
        order = torch.cat([unmasked, masked], 1).contiguous()
        pos = K.gather_rows(pos_table.detach(), order, out_dtype=tokens.dtype)     # [B, N, dd] in concatenation order
        ctx.save_for_backward(unmasked, masked, order)
        ctx.tshape = pos_table.shape
        return K.add(dec, pos)

    @staticmethod
    def backward(ctx, dy):
        unmasked, masked, order = ctx.saved_tensors
        dy = dy.contiguous()
        dd = dy.shape[2]
        dtok = K.gather_rows(dy, unmasked)
        dmask = K.colsum(K.gather_rows(dy, masked).view(-1, dd))
        dpos = torch.zeros(ctx.tshape, dtype=torch.float32, device=dy.device)
        K.scatter_add_rows_(dpos, order, dy)
        return dtok, dmask, dpos, None, None
