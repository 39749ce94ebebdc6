"""Tensor-level wrappers over the C ABI (shape checks, output/scratch allocation through
PyTorch's caching allocator, current HIP stream).  No math happens here and there is no
fallback: every function ends in a libfranken_hip.so call.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import FK_BF16, FK_F32, MASK_BLOCK_CAUSAL, MASK_CAUSAL, MASK_DENSE, MASK_KEYPAD, MASK_NONE, MASK_PREFIX, NORM_LAYER, NORM_RMS, ATTN_Q_PRESCALED, DAY_MAX_C, call, lib

Tensor = torch.Tensor


# optional live instrumentation (bench.py): name -> list of (start_event, end_event) on the launch stream
TIMERS = None
TIMER_PREFIX = None   # e.g. "attn_": only kernels whose timer name starts with it are bracketed (an event pair costs ~0.6 us of GPU time)


class _timed:
    __slots__ = ("name", "ev")

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.ev = None
        if TIMERS is not None and (TIMER_PREFIX is None or self.name.startswith(TIMER_PREFIX)):
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()

    def __exit__(self, *a):
        if self.ev is not None and TIMERS is not None:
            self.ev[1].record()
            TIMERS.setdefault(self.name, []).append(self.ev)


def fk_dtype(t) -> int:
    dt = t if isinstance(t, torch.dtype) else t.dtype
    if dt == torch.bfloat16:
        return FK_BF16
    if dt == torch.float32:
        return FK_F32
    raise TypeError(f"frankenstein_amd kernels support float32 / bfloat16, got {dt}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, device) -> Tuple[Optional[Tensor], int]:
    if nbytes == 0:
        return None, 0
    w = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return w, nbytes


def _as2d(t: Tensor) -> Tensor:
    assert t.stride(-1) == 1, "innermost dim must be contiguous"
    if t.dim() == 2:
        return t
    return t.reshape(-1, t.shape[-1])


# ------------------------------------------------------------------------------------------- GEMM
def gemm_nt(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
            res_rows: int = 0, out_dtype: Optional[torch.dtype] = None, out: Optional[Tensor] = None) -> Tensor:
    """out[M,N] = a[M,K] @ w[N,K]^T (+ bias) (+ residual[m % res_rows])."""
    assert a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1], (a.shape, w.shape)
    assert a.dtype == w.dtype and a.stride(1) == 1 and w.stride(1) == 1
    M, K = a.shape
    N = w.shape[0]
    odt = out_dtype or a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == odt
    if bias is not None:
        assert bias.dtype == a.dtype and bias.numel() == N and bias.is_contiguous()
    ldr = 0
    if residual is not None:
        assert residual.dtype == a.dtype and residual.dim() == 2 and residual.stride(1) == 1 and residual.shape[1] == N
        ldr = residual.stride(0)
    with _timed(f"gemm_nt:{M}x{N}x{K}"):
        call("fk_gemm_nt", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), M, N, K,
             _ptr(bias), _ptr(residual), ldr, res_rows, fk_dtype(a), fk_dtype(odt), _stream())
    return out


def gemv_nt(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
            ln: Optional[Tuple[Tensor, Optional[Tensor], float]] = None, act: Optional[str] = None,
            out_dtype: Optional[torch.dtype] = None, n: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """Weight-streaming skinny product for 1 <= M <= 16 rows (the single-token decode step):
    out[M,N] = act(LN(a)[M,K] @ w[:N,K]^T + bias) + residual.  ln = (gamma, beta or None, eps), act = None | "gelu";
    n < w.shape[0] uses the first n rows of a padded weight shadow (the vocabulary head)."""
    assert a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1], (a.shape, w.shape)
    assert a.dtype == w.dtype and a.stride(1) == 1 and w.stride(1) == 1
    assert act in (None, "gelu"), act
    M, K = a.shape
    N = w.shape[0] if n is None else n
    assert 0 < N <= w.shape[0], (N, w.shape)
    odt = out_dtype or a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == odt
    if bias is not None:
        assert bias.dtype == a.dtype and bias.numel() == N and bias.is_contiguous()
    ldr = 0
    if residual is not None:
        assert residual.dtype == a.dtype and residual.dim() == 2 and residual.stride(1) == 1 and residual.shape == (M, N)
        ldr = residual.stride(0)
    gamma = beta = None
    eps = 0.0
    if ln is not None:
        gamma, beta, eps = ln
        assert gamma.dtype == torch.float32 and gamma.numel() == K and gamma.is_contiguous()
        assert beta is None or (beta.dtype == torch.float32 and beta.numel() == K and beta.is_contiguous())
    with _timed(f"gemv_nt:{M}x{N}x{K}"):
        call("fk_gemv_nt", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), M, N, K,
             _ptr(bias), _ptr(residual), ldr, _ptr(gamma), _ptr(beta), float(eps), _lib.GEMV_GELU if act == "gelu" else 0,
             fk_dtype(a), fk_dtype(odt), _stream())
    return out


def gemm_nt_rope(a: Tensor, w: Tensor, bias: Optional[Tensor], table: Tensor, T: int, pos_off: int, D: int,
                 rot_cols: int, q_cols: int = 0, q_table: Optional[Tensor] = None) -> Tensor:
    """out[M,N] = a @ w^T (+ bias) with RoPE applied to the first rot_cols columns (heads of width D); rows are B x T tokens.
    q_table: table * (softmax_scale * log2 e), in the SAME allocation as table; the first q_cols columns (the queries) are rotated
    with it and so leave the projection pre-scaled for attn_fwd(..., q_prescaled=True)."""
    assert a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1] and a.dtype == w.dtype and a.stride(1) == 1 and w.stride(1) == 1
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[-1] == 2 and table.shape[-2] == D // 2
    M, Kd = a.shape
    N = w.shape[0]
    tbs = table.stride(0) if table.dim() == 4 else 0
    assert pos_off >= 0 and pos_off + T <= table.shape[-3] and M % T == 0
    out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    q_off = 0
    if q_table is not None and q_cols:
        assert q_table.shape == table.shape and q_table.dtype == torch.float32 and q_table.is_contiguous() and q_table.stride() == table.stride()
        q_off = (q_table.data_ptr() - table.data_ptr()) // 4
    else:
        q_cols = 0
    with _timed(f"gemm_nt_rope:{M}x{N}x{Kd}"):
        call("fk_gemm_nt_rope", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), N, M, N, Kd, _ptr(bias),
             table.data_ptr(), tbs, T, pos_off, D, rot_cols, q_cols, q_off, fk_dtype(a), _stream())
    return out


def gemm_nt_swiglu(a: Tensor, w13: Tensor) -> Tuple[Tensor, Tensor]:
    """(h13 [M, 2H] interleaved, g [M, H]) = fused up-projection + SwiGLU; w13 is the interleaved [2H, K] shadow."""
    assert a.dim() == 2 and w13.dim() == 2 and a.shape[1] == w13.shape[1] and a.dtype == w13.dtype
    assert a.stride(1) == 1 and w13.is_contiguous()
    M, Kd = a.shape
    H = w13.shape[0] // 2
    h13 = torch.empty((M, 2 * H), dtype=a.dtype, device=a.device)
    g = torch.empty((M, H), dtype=a.dtype, device=a.device)
    with _timed(f"gemm_nt_swiglu:{M}x{2 * H}x{Kd}"):
        call("fk_gemm_nt_swiglu", a.data_ptr(), a.stride(0), w13.data_ptr(), w13.stride(0), h13.data_ptr(), 2 * H,
             g.data_ptr(), H, M, H, Kd, fk_dtype(a), _stream())
    return h13, g


def gemm_nt_dswiglu(dy: Tensor, w2t: Tensor, h13: Tensor) -> Tensor:
    """dh13 [M, 2H] (interleaved) from dy [M, d], the transposed down-projection shadow w2t [H, d] and the saved h13."""
    assert dy.dim() == 2 and w2t.dim() == 2 and dy.shape[1] == w2t.shape[1] and dy.dtype == w2t.dtype == h13.dtype
    assert dy.stride(1) == 1 and w2t.is_contiguous() and h13.is_contiguous()
    M, Kd = dy.shape
    H = w2t.shape[0]
    assert h13.shape == (M, 2 * H)
    dh13 = torch.empty_like(h13)
    with _timed(f"gemm_nt_dswiglu:{M}x{H}x{Kd}"):
        call("fk_gemm_nt_dswiglu", dy.data_ptr(), dy.stride(0), w2t.data_ptr(), w2t.stride(0), h13.data_ptr(), 2 * H,
             dh13.data_ptr(), 2 * H, M, H, Kd, fk_dtype(dy), _stream())
    return dh13


def mlp_bwd_fused(dy: Tensor, w2t: Tensor, h13: Tensor, w13t: Tensor) -> Tuple[Tensor, Tensor]:
    """(dh13 [M, 2H], dx [M, d]) = the SwiGLU MLP's data-gradient chain in one launch (fk_mlp_bwd_fused): what gemm_nt_dswiglu(dy, w2t, h13)
    followed by gemm_nt(dh13, w13t) return, bit for bit, without reading dh13 back.  bf16, d = 384, H % 32 == 0."""
    M, d = dy.shape
    H = w2t.shape[0]
    assert dy.dtype == torch.bfloat16 == w2t.dtype == h13.dtype == w13t.dtype and dy.stride(1) == 1
    assert w2t.shape == (H, d) and w2t.is_contiguous() and h13.shape == (M, 2 * H) and h13.is_contiguous() and w13t.shape == (d, 2 * H) and w13t.is_contiguous()
    dh13 = torch.empty_like(h13)
    dx = torch.empty((M, d), dtype=dy.dtype, device=dy.device)
    with _timed(f"mlp_bwd_fused:{M}x{H}x{d}"):
        call("fk_mlp_bwd_fused", dy.data_ptr(), dy.stride(0), w2t.data_ptr(), w2t.stride(0), h13.data_ptr(), 2 * H, w13t.data_ptr(), w13t.stride(0),
             dh13.data_ptr(), 2 * H, dx.data_ptr(), d, M, H, d, fk_dtype(dy), _stream())
    return dh13, dx


# the kernels fk_gemm_nt and its fused forms choose between (fk_gemm_nt_route); NT_ROUTE_F32: fp32 operands, the staged fp32 kernel
NT_RING2, NT_RING192, NT_RING128, NT_BIG, NT_GLDS4, NT_GLDS, NT_STAGED = _lib.NT_RING2, _lib.NT_RING192, _lib.NT_RING128, _lib.NT_BIG, _lib.NT_GLDS4, _lib.NT_GLDS, _lib.NT_STAGED
NT_ROUTE_F32 = _lib.NT_ROUTE_F32
NT_LANE = _lib.NT_LANE                                     # the token-on-the-lane kernels (gemm_nt_rope_route / gemm_nt_swiglu_route only)
NT_ROUTE_NAMES = {NT_RING2: "NT_RING2", NT_RING192: "NT_RING192", NT_RING128: "NT_RING128", NT_BIG: "NT_BIG", NT_GLDS4: "NT_GLDS4",
                  NT_GLDS: "NT_GLDS", NT_STAGED: "NT_STAGED", NT_LANE: "NT_LANE", NT_ROUTE_F32: "NT_STAGED_F32"}
MLP_BWD_HIPCC, MLP_BWD_ASM = _lib.MLP_BWD_HIPCC, _lib.MLP_BWD_ASM      # fk_mlp_bwd_fused_route
MLP_BWD_ROUTE_NAMES = {MLP_BWD_HIPCC: "MLP_BWD_HIPCC", MLP_BWD_ASM: "MLP_BWD_ASM"}
TN_SMALL, TN_BIG128, TN_BIG192 = 0, 128, 192               # fk_gemm_tn_route


def gemm_nt_route(M: int, N: int, K: int, dtype=torch.bfloat16, vec_epi: bool = True, mode: int = 0, has_rope: bool = False) -> int:
    """The kernel gemm_nt (mode 0), gemm_nt_swiglu (mode 1, N = 2H), gemm_nt_dswiglu (mode 2, N = H) or gemm_nt_rope (has_rope) runs for
    this problem: one of the NT_* constants (host-side query, no launch).  vec_epi: N and the output / residual strides are multiples of
    8 and their pointers 16-byte aligned."""
    r = lib().fk_gemm_nt_route(M, N, K, fk_dtype(dtype), int(vec_epi), mode, int(has_rope))
    if r == -1:
        _lib.check(r, "fk_gemm_nt_route")
    return r


def gemm_nt_swiglu_route(M: int, H: int, K: int, lda: Optional[int] = None, ldb: Optional[int] = None, ldh: Optional[int] = None,
                         ldg: Optional[int] = None, align_ok: bool = True, dtype=torch.bfloat16) -> int:
    """The kernel gemm_nt_swiglu (fk_gemm_nt_swiglu) runs for this call: NT_LANE (the token-on-the-lane kernel) or the tiled kernel
    gemm_nt_route names for mode 1.  Leading dimensions default to the row widths; align_ok: every pointer is 16-byte aligned."""
    r = lib().fk_gemm_nt_swiglu_route(M, H, K, K if lda is None else lda, K if ldb is None else ldb, 2 * H if ldh is None else ldh,
                                      H if ldg is None else ldg, int(align_ok), fk_dtype(dtype))
    if r == -1:
        _lib.check(r, "fk_gemm_nt_swiglu_route")
    return r


def gemm_nt_rope_route(M: int, N: int, K: int, T: int, D: int, rot_cols: int, q_cols: int = 0, pos_off: int = 0, has_bias: bool = False,
                       lda: Optional[int] = None, ldb: Optional[int] = None, ldc: Optional[int] = None, align_ok: bool = True,
                       dtype=torch.bfloat16) -> int:
    """The kernel gemm_nt_rope (fk_gemm_nt_rope) runs for this call: NT_LANE or the tiled kernel gemm_nt_route names with has_rope."""
    r = lib().fk_gemm_nt_rope_route(M, N, K, K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc, int(has_bias),
                                    T, pos_off, D, rot_cols, q_cols, int(align_ok), fk_dtype(dtype))
    if r == -1:
        _lib.check(r, "fk_gemm_nt_rope_route")
    return r


def mlp_bwd_fused_route(M: int, lddh: int) -> int:
    """MLP_BWD_ASM (the generated-stream kernel) or MLP_BWD_HIPCC: the kernel mlp_bwd_fused runs for M rows of a dh13 with leading dimension lddh."""
    r = lib().fk_mlp_bwd_fused_route(M, lddh)
    if r == -1:
        _lib.check(r, "fk_mlp_bwd_fused_route")
    return r


def gemm_tn_route(M: int, N1: int, N2: int, dtype=torch.bfloat16) -> Tuple[int, int, int]:
    """(kernel, nsplit, rows_per_split) of gemm_tn for this shape: kernel is TN_SMALL, TN_BIG128 or TN_BIG192; split s sums rows
    [s * rows_per_split, min(M, (s + 1) * rows_per_split))."""
    import ctypes
    ns, rps = ctypes.c_int(0), ctypes.c_int64(0)
    r = lib().fk_gemm_tn_route(M, N1, N2, fk_dtype(dtype), ctypes.byref(ns), ctypes.byref(rps))
    if r < 0:
        _lib.check(r, "fk_gemm_tn_route")
    return r, ns.value, rps.value


def gemm_tn(a: Tensor, b: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[N1,N2] (fp32) (+)= a[M,N1]^T @ b[M,N2]."""
    assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0] and a.dtype == b.dtype
    assert a.stride(1) == 1 and b.stride(1) == 1
    M, N1 = a.shape
    N2 = b.shape[1]
    if out is None:
        assert not accumulate
        out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
    assert out.shape == (N1, N2) and out.dtype == torch.float32 and out.stride(1) == 1
    ws, nb = _ws(lib().fk_gemm_tn_workspace_bytes(M, N1, N2, fk_dtype(a)), a.device)
    with _timed(f"gemm_tn:{M}x{N1}x{N2}"):
        call("fk_gemm_tn", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N1, N2,
             int(accumulate), fk_dtype(a), _ptr(ws), nb, _stream())
    return out


def gemm_tn_swiglu_ok(a: Tensor, b: Tensor, d_up: Tensor, d_gate: Tensor) -> bool:
    """gemm_tn_swiglu_ takes this problem: a split plan (the slab reduction does the de-interleaving) and vector-aligned destinations."""
    M, N1 = a.shape
    N2 = b.shape[1]
    return (gemm_tn_route(M, N1, N2, a.dtype)[1] > 1 and N1 % 8 == 0 and N2 % 4 == 0 and d_up.is_contiguous() and d_gate.is_contiguous()
            and d_up.data_ptr() % 16 == 0 and d_gate.data_ptr() % 16 == 0)


def gemm_tn_swiglu_(a: Tensor, b: Tensor, d_up: Tensor, d_gate: Tensor) -> None:
    """d_up, d_gate ([H, N2] fp32 each) += the de-interleaved rows of a[M, 2H]^T @ b[M, N2], a's columns in the SwiGLU-interleaved
    [up 4 | gate 4] order: what gemm_tn into a temporary and two add2d_ compute, written by the slab reduction itself."""
    assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0] and a.dtype == b.dtype
    assert a.stride(1) == 1 and b.stride(1) == 1
    M, N1 = a.shape
    N2 = b.shape[1]
    for d in (d_up, d_gate):
        assert d.shape == (N1 // 2, N2) and d.dtype == torch.float32 and d.is_contiguous()
    ws, nb = _ws(lib().fk_gemm_tn_workspace_bytes(M, N1, N2, fk_dtype(a)), a.device)
    with _timed(f"gemm_tn_swiglu:{M}x{N1}x{N2}"):
        call("fk_gemm_tn_swiglu", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), d_up.data_ptr(), d_gate.data_ptr(), N2, M, N1 // 2,
             N2, fk_dtype(a), _ptr(ws), nb, _stream())


def colsum(x: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    assert x.dim() == 2 and x.stride(1) == 1
    rows, cols = x.shape
    if out is None:
        assert not accumulate
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
    assert out.numel() == cols and out.dtype == torch.float32 and out.is_contiguous()
    ws, nb = _ws(lib().fk_colsum_workspace_bytes(rows, cols), x.device)
    call("fk_colsum", x.data_ptr(), x.stride(0), out.data_ptr(), rows, cols, int(accumulate), fk_dtype(x), _ptr(ws), nb,
         _stream())
    return out


# ------------------------------------------------------------------------------------------- attention
class Mask:
    """Analytic attention mask: kind in {none, causal, block_causal(C)} with position offsets
    (the reference slices its [N,N] buffer as mask[..., -t_q:, -t_k:], models/brainformer.py:160-162)."""
    __slots__ = ("kind", "c", "q_off", "k_off", "limits", "qfirst")

    def __init__(self, kind: int = MASK_NONE, c: int = 0, q_off: int = 0, k_off: int = 0, limits=None, qfirst=None):
        self.kind, self.c, self.q_off, self.k_off, self.limits, self.qfirst = kind, c, q_off, k_off, limits, qfirst

    def sliced(self, n_full_q: int, n_full_k: int, t_q: int, t_k: int) -> "Mask":
        assert self.kind not in (MASK_PREFIX, MASK_KEYPAD, MASK_DENSE) or (n_full_q == t_q and n_full_k == t_k), "table masks cannot be sliced"
        return Mask(self.kind, self.c, self.q_off + n_full_q - t_q, self.k_off + n_full_k - t_k, self.limits, self.qfirst)

    @staticmethod
    def from_dense(mask: Tensor, t_q: int, t_k: int) -> "Mask":
        """Any boolean mask (True = attend) broadcastable to [B, H, N_q, N_k] — [N, N], [B, 1, N, N], [1, H, N, N], [B, H, N, N]: the
        reference's attention takes whatever tensor it is given and slices it as mask[..., -t_q:, -t_k:] (models/brainformer.py:160-168).
        Stored as uint8 [Bm, Hm, t_q, t_k] for the per-element path of the generic kernels (c = batch stride, q_off = head stride)."""
        assert mask.dim() >= 2
        m = mask[..., max(0, mask.shape[-2] - t_q):, max(0, mask.shape[-1] - t_k):]      # a size-1 axis stays whole, like the Python slice
        if m.dim() > 4:
            if any(d != 1 for d in m.shape[:-4]):
                raise NotImplementedError(f"dense attention mask {tuple(mask.shape)}: at most [B, H, N_q, N_k]")
            m = m.reshape(m.shape[-4:])
        while m.dim() < 4:
            m = m.unsqueeze(0)
        if m.shape[-2] not in (1, t_q) or m.shape[-1] not in (1, t_k):      # SDPA would refuse to broadcast it too
            raise ValueError(f"attention mask {tuple(mask.shape)} does not broadcast to {t_q} queries x {t_k} keys")
        m = m.expand(m.shape[0], m.shape[1], t_q, t_k)          # key-padding [B, 1, 1, N_k] and query-only [.., N_q, 1] forms: SDPA broadcasts them
        bm, hm = m.shape[0], m.shape[1]
        u8 = m.to(torch.uint8).contiguous()
        return Mask(MASK_DENSE, 0 if bm == 1 else hm * t_q * t_k, 0 if hm == 1 else t_q * t_k, 0, u8, None)

    @staticmethod
    def from_padding(q_valid: Tensor, k_valid: Tensor) -> "Mask":
        """visible(i, j) = q_valid[b, i] & k_valid[b, j]  (create_attention_mask_from_padding, models/simple_mae:228-236)."""
        return Mask(MASK_KEYPAD, 0, 0, 0, q_valid.to(torch.int32).contiguous(), k_valid.to(torch.int32).contiguous())

    @staticmethod
    def from_token_ids(q_ids: Tensor, k_ids: Tensor, block: int) -> "Mask":
        """Sub-mask of the block-causal mask at (ascending) token indices: visible(i, j) = k_ids[j] // block <= q_ids[i] // block
        (MAE.get_sub_att_matrix, models/brainformer.py:392-413), as prefix tables instead of a [B,1,n,n] tensor."""
        assert q_ids.dtype == torch.int64 and k_ids.dtype == torch.int64 and q_ids.dim() == 2 and k_ids.dim() == 2
        B, nq = q_ids.shape
        nk = k_ids.shape[1]
        limits = torch.empty((B, nq), dtype=torch.int32, device=q_ids.device)
        qfirst = torch.empty((B, nk), dtype=torch.int32, device=q_ids.device)
        call("fk_prefix_mask", q_ids.contiguous().data_ptr(), k_ids.contiguous().data_ptr(), block, limits.data_ptr(),
             qfirst.data_ptr(), B, nq, nk, _stream())
        return Mask(MASK_PREFIX, block, 0, 0, limits, qfirst)


NO_MASK = Mask()


def _bnhd(t: Tensor):
    assert t.dim() == 4 and t.stride(3) == 1 and t.stride(2) == t.shape[3], "need [B,N,H,D] with heads packed in a row"
    return t.stride(0), t.stride(1)


def _check_dense(mask: "Mask", B: int, H: int, Nq: int, Nk: int) -> None:
    """A dense table is read at b * c + h * q_off + q * Nk + k: its batch / head extents must be 1 (broadcast) or the call's."""
    if mask.kind == MASK_DENSE:
        t = mask.limits
        assert t is not None and t.dim() == 4 and t.dtype == torch.uint8 and t.is_contiguous()
        if t.shape[0] not in (1, B) or t.shape[1] not in (1, H) or t.shape[2] != Nq or t.shape[3] != Nk:
            raise ValueError(f"dense attention mask {tuple(t.shape)} does not broadcast to [B={B}, H={H}, {Nq}, {Nk}]")


def attn_fwd(q: Tensor, k: Tensor, v: Tensor, mask: Mask = NO_MASK, scale: Optional[float] = None,
             out: Optional[Tensor] = None, q_prescaled: bool = False, dropout: Optional[tuple] = None) -> Tuple[Tensor, Tensor]:
    """q [B,Nq,H,D], k/v [B,Nk,H,D] (strided views ok) -> (o [B,Nq,H,D], lse [B,H,Nq] fp32).
    q_prescaled: q already holds scale * log2(e) * q (gemm_nt_rope's q_table; bf16, D = 64 only).
    dropout = (p, seed words [2] int32 on the device, site): SDPA's dropout_p in training mode (fk_attn_fwd_dropout)."""
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    assert k.shape == (B, Nk, H, D) and v.shape == (B, Nk, H, D) and q.dtype == k.dtype == v.dtype
    _check_dense(mask, B, H, Nq, Nk)
    if out is None:
        out = torch.empty((B, Nq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    (qb, qr), (kb, kr), (vb, vr), (ob, orr) = _bnhd(q), _bnhd(k), _bnhd(v), _bnhd(out)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    with _timed(f"attn_fwd:{B}x{H}x{Nq}x{Nk}x{D}:m{mask.kind}"):
      if dropout is None:
        call("fk_attn_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, H, Nq, Nk, D,
             qb, qr, kb, kr, vb, vr, ob, orr, mask.kind, mask.c, mask.q_off, mask.k_off, _ptr(mask.limits), _ptr(mask.qfirst),
             sc, ATTN_Q_PRESCALED if q_prescaled else 0, fk_dtype(q), _stream())
      else:
        call("fk_attn_fwd_dropout", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, H, Nq, Nk, D,
             qb, qr, kb, kr, vb, vr, ob, orr, mask.kind, mask.c, mask.q_off, mask.k_off, _ptr(mask.limits), _ptr(mask.qfirst),
             sc, ATTN_Q_PRESCALED if q_prescaled else 0, dropout[0], dropout[1].data_ptr(), dropout[2], fk_dtype(q), _stream())
    return out, lse


def attn_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse: Tensor, dq: Tensor, dk: Tensor, dv: Tensor,
             mask: Mask = NO_MASK, scale: Optional[float] = None, rope_table: Optional[Tensor] = None,
             rope_off: int = 0, q_prescaled: bool = False, dropout: Optional[tuple] = None) -> None:
    """Writes dq/dk/dv (same strides as q/k/v); do must have o's strides.  rope_table: also un-rotate dq/dk (RoPE backward).
    dropout: the forward's (p, seed words, site) — the mask is regenerated, not stored."""
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    (qb, qr), (kb, kr), (vb, vr), (ob, orr) = _bnhd(q), _bnhd(k), _bnhd(v), _bnhd(o)
    assert _bnhd(dq) == (qb, qr) and _bnhd(dk) == (kb, kr) and _bnhd(dv) == (vb, vr) and _bnhd(do) == (ob, orr)
    assert do.dtype == q.dtype and dq.dtype == q.dtype
    _check_dense(mask, B, H, Nq, Nk)
    delta = torch.empty(2 * B * H * ((Nq + 63) // 64 * 64), dtype=torch.float32, device=q.device)     # scratch: row statistics for dK/dV
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    with _timed(f"attn_bwd:{B}x{H}x{Nq}x{Nk}x{D}:m{mask.kind}"):
      head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(),
              dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, H, Nq, Nk, D, qb, qr, kb, kr, vb, vr, ob, orr,
              mask.kind, mask.c, mask.q_off, mask.k_off, _ptr(mask.limits), _ptr(mask.qfirst), sc, _ptr(rope_table),
              0 if rope_table is None or rope_table.dim() == 3 else rope_table.stride(0), rope_off,
              ATTN_Q_PRESCALED if q_prescaled else 0)
      if dropout is None:
        call("fk_attn_bwd", *head, fk_dtype(q), _stream())
      else:
        call("fk_attn_bwd_dropout", *head, dropout[0], dropout[1].data_ptr(), dropout[2], fk_dtype(q), _stream())


# the kernels fk_attn_fwd / fk_attn_bwd choose between (fk_attn_route), one table per launch: forward, dQ, dK/dV
ATTN_FWD_ROUTE_NAMES = {_lib.ATTN_FWD_GENERIC: "FWD_GENERIC", _lib.ATTN_FWD_FEWQ: "FWD_FEWQ", _lib.ATTN_FWD_PS: "FWD_PS", _lib.ATTN_FWD_ASM: "FWD_ASM"}
ATTN_DQ_ROUTE_NAMES = {_lib.ATTN_DQ_GENERIC: "DQ_GENERIC", _lib.ATTN_DQ_FEWQ: "DQ_FEWQ", _lib.ATTN_DQ_PS: "DQ_PS", _lib.ATTN_DQ_ASM: "DQ_ASM"}
ATTN_DKDV_ROUTE_NAMES = {_lib.ATTN_DKDV_GENERIC: "DKDV_GENERIC", _lib.ATTN_DKDV_PS: "DKDV_PS", _lib.ATTN_DKDV_ASM: "DKDV_ASM", _lib.ATTN_DKDVW_ASM: "DKDVW_ASM"}


def attn_route(Nq: int, Nk: int, D: int, dtype=torch.bfloat16, mask: Mask = NO_MASK, q_prescaled: bool = False, dropout: bool = False,
               rope: bool = False) -> Tuple[int, int, int]:
    """(fwd, dq, dkdv): the kernels attn_fwd and attn_bwd run for this problem, keys of ATTN_FWD_ / ATTN_DQ_ / ATTN_DKDV_ROUTE_NAMES
    (host-side query, no launch; the launchers ask the same function).  dropout: a dropout tuple is passed; rope: attn_bwd gets a
    rope_table."""
    import ctypes
    f, q, kv = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    call("fk_attn_route", Nq, Nk, D, fk_dtype(dtype), mask.kind, mask.c, mask.q_off, mask.k_off, ATTN_Q_PRESCALED if q_prescaled else 0,
         int(dropout), int(rope), ctypes.byref(f), ctypes.byref(q), ctypes.byref(kv))
    return f.value, q.value, kv.value


def attn_route_names(*args, **kw) -> Tuple[str, str, str]:
    f, q, kv = attn_route(*args, **kw)
    return ATTN_FWD_ROUTE_NAMES[f], ATTN_DQ_ROUTE_NAMES[q], ATTN_DKDV_ROUTE_NAMES[kv]


def attn_combine(parts: Tensor, lse_parts: Optional[Tensor] = None, want_lse: bool = True):
    """parts [B, S, T, H, D] (+ lse_parts [B, S, H, T]) -> (out [B, T, H, D], lse [B, H, T] or None): fk_attn_combine."""
    B, S, T, H, D = parts.shape
    assert parts.is_contiguous()
    out = torch.empty((B, T, H, D), dtype=parts.dtype, device=parts.device)
    lse = None
    if lse_parts is not None:
        assert lse_parts.dtype == torch.float32 and lse_parts.is_contiguous() and lse_parts.shape == (B, S, H, T)
        lse = torch.empty((B, H, T), dtype=torch.float32, device=parts.device) if want_lse else None
    call("fk_attn_combine", parts.data_ptr(), _ptr(lse_parts), out.data_ptr(), _ptr(lse), B, S, T, H, D, fk_dtype(parts), _stream())
    return out, lse


# ------------------------------------------------------------------------------------------- norms
def norm_fwd(x: Tensor, gamma: Tensor, beta: Optional[Tensor], eps: float, kind: int = NORM_LAYER):
    x2 = _as2d(x)
    assert x2.is_contiguous() and gamma.dtype == torch.float32
    rows, dim = x2.shape
    y = torch.empty_like(x2)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    call("fk_norm_fwd", x2.data_ptr(), gamma.data_ptr(), _ptr(beta), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
         rows, dim, eps, kind, fk_dtype(x), _stream())
    return y.view(x.shape), mean, rstd


def norm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor] = None,
             kind: int = NORM_LAYER, want_beta: bool = True, dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None,
             accumulate: bool = False):
    """returns (dx, dgamma, dbeta) with dx = dres + norm_bwd(dy); given dgamma / dbeta buffers are written (+= when accumulate)."""
    x2, dy2 = _as2d(x), _as2d(dy)
    assert x2.is_contiguous() and dy2.is_contiguous() and dy2.dtype == x2.dtype
    rows, dim = x2.shape
    dx = torch.empty_like(x2)
    if dgamma is None:
        assert not accumulate
        dgamma = torch.empty(dim, dtype=torch.float32, device=x.device)
    if dbeta is None and want_beta:
        assert not accumulate
        dbeta = torch.empty(dim, dtype=torch.float32, device=x.device)
    if not want_beta:
        dbeta = None
    for t in (dgamma, dbeta):
        assert t is None or (t.dtype == torch.float32 and t.numel() == dim and t.is_contiguous())
    dres2 = None
    if dres is not None:
        dres2 = _as2d(dres)
        assert dres2.is_contiguous() and dres2.dtype == x2.dtype
    ws, nb = _ws(lib().fk_norm_bwd_workspace_bytes(rows, dim), x.device)
    call("fk_norm_bwd", dy2.data_ptr(), x2.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(dres2),
         dx.data_ptr(), dgamma.data_ptr(), _ptr(dbeta), rows, dim, kind, int(accumulate), fk_dtype(x), _ptr(ws), nb, _stream())
    return dx.view(x.shape), dgamma, dbeta


# ------------------------------------------------------------------------------------------- pointwise
def rope_(x: Tensor, nheads: int, D: int, table: Tensor, pos_off: int = 0, conj: bool = False) -> Tensor:
    """In place on the first nheads*D columns of each row of x [B,T,ld]; table fp32 [Tc, D/2, 2] or [B, Tc, D/2, 2]."""
    assert x.dim() == 3 and x.stride(2) == 1 and x.stride(0) == x.shape[1] * x.stride(1)
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[-1] == 2 and table.shape[-2] == D // 2
    B, T, _ = x.shape
    tbs = 0
    if table.dim() == 4:
        assert table.shape[0] == B
        tbs = table.stride(0)
    assert pos_off >= 0 and pos_off + T <= table.shape[-3], "rope cache shorter than the sequence"
    call("fk_rope", x.data_ptr(), B, T, x.stride(1), nheads, D, table.data_ptr(), tbs, pos_off, int(conj), fk_dtype(x), _stream())
    return x


def patchify(x: Tensor, P: int, ldp: int, dtype: torch.dtype) -> Tensor:
    assert x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
    B, T, Cc = x.shape
    tok = torch.empty((B * (T // P) * Cc, ldp), dtype=dtype, device=x.device)
    call("fk_patchify", x.data_ptr(), tok.data_ptr(), B, T, Cc, P, ldp, fk_dtype(dtype), _stream())
    return tok


def _day_check(x: Tensor, day: Optional[Tensor], delta: Tensor, bias: Tensor):
    assert x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
    B, T, Cc = x.shape
    n_days = delta.shape[0]
    assert delta.dtype == torch.float32 and delta.shape == (n_days, Cc, Cc) and delta.is_contiguous() and delta.device == x.device
    assert bias.dtype == torch.float32 and bias.shape == (n_days, Cc) and bias.is_contiguous() and bias.device == x.device
    assert day is None or (day.dtype == torch.int64 and day.shape == (B,) and day.is_contiguous() and day.device == x.device)
    return B, T, Cc, n_days


def day_adapter_fwd(x: Tensor, day: Optional[Tensor], delta: Tensor, bias: Tensor, P: int, ldp: int, dtype: torch.dtype) -> Tensor:
    """fk_day_adapter_fwd: tok [B * (T / P) * C, ldp] = patchify(x + x @ delta[day] + bias[day]); day int64 [B] on the device (None, or
    an entry outside [0, n_days): pass-through).  P = 1, ldp = 1, float32 is the adapted [B, T, C] signal itself."""
    B, T, Cc, n_days = _day_check(x, day, delta, bias)
    tok = torch.empty((B * (T // P) * Cc, ldp), dtype=dtype, device=x.device)
    with _timed("day_adapter_fwd"):
        call("fk_day_adapter_fwd", x.data_ptr(), _ptr(day), delta.data_ptr(), bias.data_ptr(), tok.data_ptr(), B, T, Cc, P, ldp, n_days,
             fk_dtype(dtype), _stream())
    return tok


def day_adapter_bwd(x: Tensor, day: Optional[Tensor], d_tok: Tensor, P: int, delta_shape, out: Optional[Tuple[Tensor, Tensor]] = None):
    """fk_day_adapter_bwd: (d_delta [n_days, C, C], d_bias [n_days, C]) from d_tok fp32 [B * (T / P) * C, ldp]; every slice is
    overwritten (a day absent from the batch: zeros)."""
    assert x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
    B, T, Cc = x.shape
    n_days = delta_shape[0]
    assert tuple(delta_shape) == (n_days, Cc, Cc)
    assert day is None or (day.dtype == torch.int64 and day.shape == (B,) and day.is_contiguous() and day.device == x.device)
    assert d_tok.dtype == torch.float32 and d_tok.dim() == 2 and d_tok.is_contiguous() and d_tok.shape[0] == B * (T // P) * Cc
    ldp = d_tok.shape[1]
    if out is None:
        out = (torch.empty((n_days, Cc, Cc), dtype=torch.float32, device=x.device), torch.empty((n_days, Cc), dtype=torch.float32, device=x.device))
    d_delta, d_bias = out
    assert d_delta.shape == (n_days, Cc, Cc) and d_bias.shape == (n_days, Cc) and d_delta.is_contiguous() and d_bias.is_contiguous()
    assert d_delta.dtype == torch.float32 and d_bias.dtype == torch.float32
    ws, nb = _ws(lib().fk_day_adapter_bwd_workspace_bytes(B, T, Cc, P, n_days) if day is not None else 0, x.device)
    with _timed("day_adapter_bwd"):
        call("fk_day_adapter_bwd", x.data_ptr(), _ptr(day), d_tok.data_ptr(), ldp, d_delta.data_ptr(), d_bias.data_ptr(), _ptr(ws), nb,
             B, T, Cc, P, n_days, _stream())
    return d_delta, d_bias


def augment_cfg_struct(cfg) -> _lib.AugmentCfg:
    """fk_augment_cfg from an object with the knobs as attributes (engine.AugmentConfig)"""
    return _lib.AugmentCfg(float(cfg.white_sd), float(cfg.offset_sd), float(cfg.chan_drop_p), int(cfg.time_shift), int(cfg.n_time_masks),
                      int(cfg.time_mask_len), int(bool(cfg.keep_padding)), 0)


def augment_patchify(x: Tensor, P: int, ldp: int, dtype: torch.dtype, cfg, words: Tensor) -> Tensor:
    """fk_augment_patchify: tok [B * (T / P) * C, ldp] = patchify(augment(x)), drawn with the device words int32 [seed, step] (the rule:
    include/franken_hip.h).  With every knob zero: fk_patchify's bits.  P = 1, ldp = 1, float32 is the augmented [B, T, C] signal itself."""
    assert x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
    assert words.dtype == torch.int32 and words.shape == (2,) and words.is_contiguous() and words.device == x.device
    B, T, Cc = x.shape
    c = augment_cfg_struct(cfg)
    tok = torch.empty((B * (T // P) * Cc, ldp), dtype=dtype, device=x.device)
    with _timed("augment_patchify"):
        call("fk_augment_patchify", x.data_ptr(), tok.data_ptr(), B, T, Cc, P, ldp, ctypes.byref(c), words.data_ptr(), fk_dtype(dtype), _stream())
    return tok


# ------------------------------------------------------------------------------------------- low-rank adapters (csrc/lora.hip)
def lora_route(M: int, N: int, K: int, r: int, dtype) -> int:
    """fk_lora_route: the forward's kernel variant (_lib.LORA_R32 / LORA_R64), or -1 outside the envelope"""
    return lib().fk_lora_route(M, N, K, r, dtype if isinstance(dtype, int) else fk_dtype(dtype))


def lora_fwd(x: Tensor, a: Tensor, b: Tensor, scale: float, res: Optional[Tensor] = None, out: Optional[Tensor] = None,
             q_cols: int = 0, q_scale: float = 1.0, want_u: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """fk_lora_fwd: (out, u) with u [M, r] = round(x a^T) and out [M, N] = (res or 0) + scale * colscale * (u b^T); a [r, K], b [N, r] in
    x's dtype.  res may be `out` itself (in place).  The data gradient is lora_fwd(dy, b_t, a_t, scale, res=dh, out=dh)."""
    assert x.dim() == 2 and x.stride(1) == 1 and a.dim() == 2 and b.dim() == 2 and a.is_contiguous() and b.is_contiguous()
    assert a.dtype == x.dtype and b.dtype == x.dtype
    M, K = x.shape
    r, N = a.shape[0], b.shape[0]
    assert a.shape == (r, K) and b.shape == (N, r), (x.shape, a.shape, b.shape)
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == x.dtype
    ldr = 0
    if res is not None:
        assert res.shape == (M, N) and res.stride(1) == 1 and res.dtype == x.dtype
        ldr = res.stride(0)
    u = torch.empty((M, r), dtype=x.dtype, device=x.device) if want_u else None
    with _timed(f"lora_fwd:{M}x{N}x{K}x{r}"):
        call("fk_lora_fwd", x.data_ptr(), x.stride(0), a.data_ptr(), b.data_ptr(), M, N, K, r, scale, q_cols, q_scale, _ptr(res), ldr,
             _ptr(u), out.data_ptr(), out.stride(0), fk_dtype(x), _stream())
    return out, u


def lora_wgrad(dy: Tensor, u: Tensor, du: Tensor, x: Tensor, scale: float, dA: Optional[Tensor] = None, dB: Optional[Tensor] = None,
               accumulate: bool = False) -> Tuple[Tensor, Tensor]:
    """fk_lora_wgrad: dB [N, r] (+)= scale * dy^T u and dA [r, K] (+)= scale * du^T x in fp32, du the unscaled dy b of the transposed
    lora_fwd call; the row slices are added in a fixed order (same bits on every run)."""
    assert dy.dim() == 2 and x.dim() == 2 and dy.is_contiguous() and x.is_contiguous() and u.is_contiguous() and du.is_contiguous()
    M, N = dy.shape
    K, r = x.shape[1], u.shape[1]
    assert x.shape[0] == M and u.shape == (M, r) and du.shape == (M, r) and dy.dtype == x.dtype == u.dtype == du.dtype
    if dA is None or dB is None:
        assert not accumulate and dA is None and dB is None
        dA = torch.empty((r, K), dtype=torch.float32, device=x.device)
        dB = torch.empty((N, r), dtype=torch.float32, device=x.device)
    assert dA.shape == (r, K) and dB.shape == (N, r) and dA.dtype == dB.dtype == torch.float32 and dA.is_contiguous() and dB.is_contiguous()
    ws, nb = _ws(lib().fk_lora_wgrad_workspace_bytes(M, N, K, r), x.device)
    with _timed(f"lora_wgrad:{M}x{N}x{K}x{r}"):
        call("fk_lora_wgrad", dy.data_ptr(), u.data_ptr(), du.data_ptr(), x.data_ptr(), M, N, K, r, scale, dA.data_ptr(), dB.data_ptr(),
             int(accumulate), fk_dtype(x), _ptr(ws), nb, _stream())
    return dA, dB


def lora_merge(w: Tensor, a: Tensor, b: Tensor, scale: float, out_dtype: Optional[torch.dtype] = None, out: Optional[Tensor] = None) -> Tensor:
    """fk_lora_merge: out [N, K] = w + scale * (b a) from the fp32 masters, an fp32 fma chain over r; out_dtype float32 (may be w itself)
    or bfloat16 (the rounding of that same fp32 value)."""
    assert w.dim() == 2 and w.is_contiguous() and a.is_contiguous() and b.is_contiguous()
    assert w.dtype == a.dtype == b.dtype == torch.float32
    N, K = w.shape
    r = a.shape[0]
    assert a.shape == (r, K) and b.shape == (N, r)
    odt = out_dtype or (out.dtype if out is not None else torch.float32)
    if out is None:
        out = torch.empty((N, K), dtype=odt, device=w.device)
    assert out.shape == (N, K) and out.stride(1) == 1 and out.dtype == odt
    with _timed("lora_merge"):
        call("fk_lora_merge", w.data_ptr(), a.data_ptr(), b.data_ptr(), N, K, r, scale, out.data_ptr(), out.stride(0), fk_dtype(odt), _stream())
    return out


def swiglu_fwd(h13: Tensor) -> Tensor:
    assert h13.dim() == 2 and h13.is_contiguous()
    rows, H2 = h13.shape
    g = torch.empty((rows, H2 // 2), dtype=h13.dtype, device=h13.device)
    call("fk_swiglu_fwd", h13.data_ptr(), g.data_ptr(), rows, H2 // 2, fk_dtype(h13), _stream())
    return g


def swiglu_bwd(h13: Tensor, dg: Tensor) -> Tensor:
    assert h13.is_contiguous() and dg.is_contiguous()
    rows, H2 = h13.shape
    d = torch.empty_like(h13)
    call("fk_swiglu_bwd", h13.data_ptr(), dg.data_ptr(), d.data_ptr(), rows, H2 // 2, fk_dtype(h13), _stream())
    return d


def gelu_fwd(x: Tensor) -> Tensor:
    assert x.is_contiguous()
    y = torch.empty_like(x)
    call("fk_gelu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), fk_dtype(x), _stream())
    return y


def dropout(x: Tensor, p: float, seed: Tensor, site: int, residual: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """y = [residual +] keep ? x / (1 - p) : 0 (fk_dropout; nn.Dropout in training mode).  seed: int32 [2] on the device (seed, step).
    The backward is the same call on dy (same p / seed / site) without residual."""
    assert x.is_contiguous() and (residual is None or (residual.is_contiguous() and residual.shape == x.shape and residual.dtype == x.dtype))
    assert seed.dtype == torch.int32 and seed.numel() == 2 and seed.device == x.device
    y = torch.empty_like(x) if out is None else out
    call("fk_dropout", x.data_ptr(), _ptr(residual), y.data_ptr(), x.numel(), p, seed.data_ptr(), site, fk_dtype(x), _stream())
    return y


def gelu_bwd(x: Tensor, dy: Tensor) -> Tensor:
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x)
    call("fk_gelu_bwd", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), fk_dtype(x), _stream())
    return dx


def cast_pack(src: Tensor, dst: Tensor, transpose: bool = False) -> Tensor:
    """dst[r, c] = src[r, c] (or dst[c, r]) ; src fp32 [rows, cols], dst pre-allocated (may be wider: zero padded by caller)."""
    assert src.dtype == torch.float32 and src.dim() == 2 and src.stride(1) == 1 and dst.dim() == 2 and dst.stride(1) == 1
    rows, cols = src.shape
    call("fk_cast_pack", src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), rows, cols, int(transpose),
         fk_dtype(dst), _stream())
    return dst


def cast_pack_rows(src: Tensor, dst: Tensor, transpose: bool, rblk: int, rstride: int, roff: int) -> Tensor:
    """cast_pack with the row map j -> (j // rblk) * rstride + j % rblk + roff (interleaved SwiGLU weight shadows)."""
    assert src.dtype == torch.float32 and src.dim() == 2 and src.stride(1) == 1 and dst.dim() == 2 and dst.stride(1) == 1
    rows, cols = src.shape
    call("fk_cast_pack_rows", src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), rows, cols, int(transpose),
         rblk, rstride, roff, fk_dtype(dst), _stream())
    return dst


def cast_pack_multi(jobs: Tensor, njobs: int, total_chunks: int, dtype: torch.dtype) -> None:
    """jobs: device uint8 tensor holding njobs fk_pack_job records (see include/franken_hip.h)."""
    assert jobs.dtype == torch.uint8 and jobs.is_cuda and jobs.numel() >= 64 * njobs
    call("fk_cast_pack_multi", jobs.data_ptr(), njobs, total_chunks, fk_dtype(dtype), _stream())


def cast(src: Tensor, dtype: torch.dtype) -> Tensor:
    assert src.is_contiguous()
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    call("fk_cast", src.data_ptr(), fk_dtype(src), dst.data_ptr(), fk_dtype(dtype), src.numel(), _stream())
    return dst


def add(a: Tensor, b: Tensor) -> Tensor:
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and a.dtype == b.dtype
    y = torch.empty_like(a)
    call("fk_add", a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), fk_dtype(a), _stream())
    return y


def gather_rows(src: Tensor, idx: Tensor, out_dtype: Optional[torch.dtype] = None, idx_mod: int = 0) -> Tensor:
    """out[b, i, :] = src[b, idx[b,i] (% idx_mod), :]; src [B, N, W] or a shared table [N, W]; idx int64 [B, n]."""
    assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.is_contiguous() and src.is_contiguous()
    B, n = idx.shape
    W = src.shape[-1]
    sbs = src.shape[-2] * W if src.dim() == 3 else 0
    assert src.dim() == 2 or src.shape[0] == B
    odt = out_dtype or src.dtype
    out = torch.empty((B, n, W), dtype=odt, device=src.device)
    call("fk_gather_rows", src.data_ptr(), sbs, fk_dtype(src), idx.data_ptr(), idx_mod, out.data_ptr(), n * W, fk_dtype(odt),
         B, n, W, 0, _stream())
    return out


def scatter_rows_(dst: Tensor, idx: Tensor, src: Tensor) -> Tensor:
    """dst[b, idx[b,i], :] = src[b, i, :]   (dst [B, N, W] contiguous, updated in place)."""
    assert idx.dtype == torch.int64 and idx.is_contiguous() and src.is_contiguous() and dst.is_contiguous()
    B, n = idx.shape
    W = src.shape[-1]
    assert src.shape == (B, n, W) and dst.dim() == 3 and dst.shape[0] == B and dst.shape[2] == W
    call("fk_gather_rows", src.data_ptr(), n * W, fk_dtype(src), idx.data_ptr(), 0, dst.data_ptr(), dst.shape[1] * W,
         fk_dtype(dst), B, n, W, 1, _stream())
    return dst


def scatter_add_rows_(table: Tensor, idx: Tensor, src: Tensor, idx_mod: int = 0) -> Tensor:
    """table[idx[r] (% idx_mod), :] += src[r, :]  (fp32 table; atomics)."""
    assert table.dtype == torch.float32 and table.is_contiguous() and src.is_contiguous() and idx.is_contiguous()
    W = table.shape[-1]
    rows = idx.numel()
    assert src.numel() == rows * W
    call("fk_scatter_add_rows", src.data_ptr(), fk_dtype(src), idx.data_ptr(), idx_mod, table.data_ptr(), rows, W, _stream())
    return table


def copy2d(src: Tensor, dst: Tensor) -> Tensor:
    assert src.dim() == 2 and dst.shape == src.shape and src.stride(1) == 1 and dst.stride(1) == 1 and src.dtype == dst.dtype
    call("fk_copy2d", src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), src.shape[0], src.shape[1],
         fk_dtype(src), _stream())
    return dst


def add2d_(dst: Tensor, src: Tensor) -> Tensor:
    """dst += src  (fp32 2-D, row strides allowed)."""
    assert dst.dtype == torch.float32 and src.dtype == torch.float32 and dst.shape == src.shape and dst.dim() == 2
    assert dst.stride(1) == 1 and src.stride(1) == 1
    call("fk_add2d", src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), dst.shape[0], dst.shape[1], _stream())
    return dst


# ------------------------------------------------------------------------------------------- decode step (device-side position)
def gpt_embed_step(idx: Tensor, wte: Tensor, wpe: Tensor, pos: Tensor, dtype: torch.dtype) -> Tensor:
    """x[b] = wte[idx[b]] + wpe[pos[0]]; idx int64 [B], pos int32 [1] on the device."""
    assert idx.dtype == torch.int64 and idx.is_contiguous() and pos.dtype == torch.int32 and pos.numel() == 1
    assert wte.dtype == torch.float32 and wpe.dtype == torch.float32 and wte.is_contiguous() and wpe.is_contiguous()
    B, dim = idx.numel(), wte.shape[1]
    out = torch.empty((B, dim), dtype=dtype, device=idx.device)
    call("fk_gpt_embed_step", idx.data_ptr(), wte.data_ptr(), wpe.data_ptr(), pos.data_ptr(), out.data_ptr(), B, dim, wte.shape[0],
         fk_dtype(dtype), _stream())
    return out


def kv_append_(qkv: Tensor, kv: Tensor, pos: Tensor) -> None:
    """kv[b, pos[0], :] = qkv[b, d:3d]; qkv [B, 3d] contiguous, kv [B, Tmax, 2d] contiguous."""
    B, d3 = qkv.shape
    assert qkv.is_contiguous() and kv.is_contiguous() and kv.shape[0] == B and kv.shape[2] * 3 == d3 * 2 and kv.dtype == qkv.dtype
    call("fk_kv_append", qkv.data_ptr(), kv.data_ptr(), pos.data_ptr(), B, d3 // 3, kv.shape[1], fk_dtype(qkv), _stream())


class SampleState:
    """Device-side state of fk_sample_topk: Philox seed, step counter (= column of `out` the next draw goes to), ticket word."""

    def __init__(self, device, seed: Optional[int] = None, step: int = 0):
        if seed is None:                                   # follows torch.manual_seed like torch.multinomial would
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.seed = torch.tensor([seed], dtype=torch.int64, device=device)
        self.step = torch.tensor([step], dtype=torch.int64, device=device)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)


def _sample_topk_call(fn: str, logits: Tensor, temperature: float, top_k: Optional[int], state: SampleState, cur: Optional[Tensor],
                      out: Optional[Tensor], pos_inc: Optional[Tensor], *tail, top_p: Optional[float] = None) -> Tensor:
    """The body of sample_topk / sample_topk_eos / sample_topp: the asserts and the call of `fn`; `tail` = its arguments behind the ticket,
    top_p (sample_topp only) = its argument behind top_k."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    B, V = logits.shape
    if cur is None:
        cur = torch.empty(B, dtype=torch.int64, device=logits.device)
    assert cur.dtype == torch.int64 and cur.is_contiguous() and cur.numel() == B
    out_ld = out_cols = 0
    if out is not None:
        assert out.dtype == torch.int64 and out.dim() == 2 and out.shape[0] == B and out.stride(1) == 1
        out_ld, out_cols = out.stride(0), out.shape[1]          # the kernel stops writing at column out_cols, whatever the step counter says
    if pos_inc is not None:
        assert pos_inc.dtype == torch.int32 and pos_inc.numel() == 1
    nucleus = () if top_p is None else (float(top_p),)
    call(fn, logits.data_ptr(), logits.stride(0), B, V, float(temperature), int(top_k or 0), *nucleus, state.seed.data_ptr(), state.step.data_ptr(),
         _ptr(pos_inc), cur.data_ptr(), _ptr(out), out_ld, out_cols, state.ticket.data_ptr(), *tail, _stream())
    return cur


def sample_topk(logits: Tensor, temperature: float, top_k: Optional[int], state: SampleState, cur: Optional[Tensor] = None,
                out: Optional[Tensor] = None, pos_inc: Optional[Tensor] = None) -> Tensor:
    """One token per row of fp32 logits [B, V] (row stride >= V): temperature, top-k crop, softmax, multinomial — one launch
    (models/gpt2_model.py:340-351).  Writes cur [B] int64 (returned), out[:, step] if given, then step += 1 (and pos_inc += 1)."""
    return _sample_topk_call("fk_sample_topk", logits, temperature, top_k, state, cur, out, pos_inc)


class SampleEosState:
    """End-of-text state of sample_topk_eos for B rows: done [B] int32 0/1, len [B] int32 (generated tokens, the end-of-text token counted
    once), the accumulator word live_acc and live [1] int32 = the rows not done after the last step."""

    def __init__(self, device, rows: int, eos: Optional[int]):
        self.eos = -1 if eos is None else int(eos)
        self.done = torch.zeros(rows, dtype=torch.int32, device=device)
        self.len = torch.zeros(rows, dtype=torch.int32, device=device)
        self.live_acc = torch.zeros(1, dtype=torch.int32, device=device)
        self.live = torch.full((1,), rows, dtype=torch.int32, device=device)


def sample_topk_eos(logits: Tensor, temperature: float, top_k: Optional[int], state: SampleState, eos_state: SampleEosState,
                    cur: Optional[Tensor] = None, out: Optional[Tensor] = None, pos_inc: Optional[Tensor] = None) -> Tensor:
    """sample_topk with an end-of-text id (fk_sample_topk_eos): a done row emits eos_state.eos and draws nothing, every other row draws
    what sample_topk draws with the same seed and step, its length grows by one, and a row that draws the id becomes done;
    eos_state.live[0] = the rows still not done."""
    assert eos_state.done.numel() == logits.shape[0] and eos_state.len.numel() == logits.shape[0]
    return _sample_topk_call("fk_sample_topk_eos", logits, temperature, top_k, state, cur, out, pos_inc, eos_state.eos, eos_state.done.data_ptr(),
                             eos_state.len.data_ptr(), eos_state.live_acc.data_ptr(), eos_state.live.data_ptr())


def sample_topp(logits: Tensor, temperature: float, top_k: Optional[int], top_p: float, state: SampleState,
                eos_state: Optional[SampleEosState] = None, cur: Optional[Tensor] = None, out: Optional[Tensor] = None,
                pos_inc: Optional[Tensor] = None) -> Tensor:
    """sample_topk with a nucleus crop behind the top-k crop, still one launch (fk_sample_topp): of the tokens the top-k crop keeps, token i
    stays iff the tokens with a strictly larger logit hold less than top_p of the kept probability; so the most likely token always stays,
    equal logits stay or go together, and top_p = 1 draws what sample_topk draws with the same seed and step.  eos_state: the end-of-text
    rules of sample_topk_eos on top.  0 < top_p <= 1."""
    assert 0.0 < float(top_p) <= 1.0, f"top_p {top_p} outside (0, 1]"
    if eos_state is None:
        tail = (-1, None, None, None, None)                # the plain mode: no end-of-text state, the id is not read
    else:
        assert eos_state.done.numel() == logits.shape[0] and eos_state.len.numel() == logits.shape[0]
        tail = (eos_state.eos, eos_state.done.data_ptr(), eos_state.len.data_ptr(), eos_state.live_acc.data_ptr(), eos_state.live.data_ptr())
    return _sample_topk_call("fk_sample_topp", logits, temperature, top_k, state, cur, out, pos_inc, *tail, top_p=top_p)


LOGIT_RULES_MAX_HISTORY = 4096                  # the envelope of fk_logit_rules: prompt + new tokens of a row


def inv_penalty(penalty: float):
    """(p, 1 / p) as the fp32 values fk_logit_rules multiplies by: p rounded to fp32, 1 / p computed in float64 and rounded once."""
    p = torch.tensor(float(penalty), dtype=torch.float32)
    return float(p), float((1.0 / p.double()).to(torch.float32))


class LogitRules:
    """The rules of fk_logit_rules and the device-side token history they read: repetition_penalty p (with inv_p, both fp32 values),
    no_repeat_ngram_size n, min_new_tokens m, the end-of-text id e (-1: none), and hist int32 [rows, t0 + steps] whose first t0 columns
    hold `prompt` (int64 [S, t0]) and which the kernel appends to.  width = W: the state of a beam search, rows = S * W (every beam of a
    sentence starts from its prompt) and a second buffer hist2, swapped with hist by the parity of the step."""

    def __init__(self, prompt: Tensor, steps: int, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
                 eos: Optional[int] = None, width: Optional[int] = None):
        assert prompt.dim() == 2
        S, t0 = prompt.shape
        assert t0 + steps <= LOGIT_RULES_MAX_HISTORY, f"fk_logit_rules holds histories of up to {LOGIT_RULES_MAX_HISTORY} tokens, got {t0 + steps}"
        self.p, self.inv_p = inv_penalty(repetition_penalty)
        self.n, self.m, self.e = int(no_repeat_ngram_size), int(min_new_tokens), -1 if eos is None else int(eos)
        self.t0, self.steps, self.width = t0, int(steps), width
        rows = S * (width or 1)
        self.hist = torch.empty((rows, t0 + self.steps), dtype=torch.int32, device=prompt.device)
        self.hist[:, :t0] = prompt.to(torch.int32) if width is None else prompt.to(torch.int32).repeat_interleave(width, dim=0)
        self.hist2 = None if width is None else torch.empty_like(self.hist)


def logit_rules_(logits: Tensor, rules: LogitRules, step: Tensor, cur: Tensor, parent_log: Optional[Tensor] = None, broadcast: bool = False) -> Tensor:
    """Repetition penalty, n-gram ban and minimum length on fp32 logits [R, V] (row stride >= V) in place, one launch in front of the
    sampling / beam_topk launch (fk_logit_rules has the rule).  step int64 [1]: the device-side count of generated tokens (SampleState.step,
    BeamState.step); cur int64 [rows]: the tokens of the previous step, which the kernel appends to rules.hist before it applies the rules.
    Beam mode (rules.width = W, parent_log = BeamState.parent_log): the histories follow the parents of the last select; broadcast=True is
    the first step, logits [S, V], one row per sentence."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    R, V = logits.shape
    rows = rules.hist.shape[0]
    assert step.dtype == torch.int64 and step.numel() == 1
    assert cur.dtype == torch.int64 and cur.is_contiguous() and cur.numel() == rows
    assert rules.hist.dtype == torch.int32 and rules.hist.stride(1) == 1
    if rules.width is None:
        assert parent_log is None and not broadcast and R == rows
        tail = (None, 0, 0, 0)
        hist2 = None
    else:
        W = rules.width
        assert parent_log is not None and parent_log.dtype == torch.int32 and parent_log.dim() == 2 and parent_log.is_contiguous()
        assert parent_log.shape[1] == rows and R == (rows // W if broadcast else rows)
        assert rules.hist2.shape == rules.hist.shape and rules.hist2.stride() == rules.hist.stride()
        tail = (parent_log.data_ptr(), parent_log.shape[0], W, int(bool(broadcast)))
        hist2 = rules.hist2
    call("fk_logit_rules", logits.data_ptr(), logits.stride(0), R, V, rules.p, rules.n, rules.m, rules.e, step.data_ptr(), cur.data_ptr(),
         rules.hist.data_ptr(), _ptr(hist2), rules.hist.stride(0), rules.t0, rules.steps, *tail, _stream())
    return logits


def attn_decode(qkv: Tensor, kv: Tensor, pos: Tensor, n_head: int) -> Tensor:
    """one causal query per sample against the cache rows 0..pos[0]: q = qkv[:, :d] -> o [B, d]."""
    B, d3 = qkv.shape
    d = d3 // 3
    D = d // n_head
    out = torch.empty((B, d), dtype=qkv.dtype, device=qkv.device)
    call("fk_attn_decode", qkv.data_ptr(), qkv.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), out.data_ptr(), d, pos.data_ptr(),
         B, n_head, D, 1.0 / math.sqrt(D), fk_dtype(qkv), _stream())
    return out


# ------------------------------------------------------------------------------------------- beam search on the caches
BEAM_MAX_WIDTH, BEAM_MAX_TOPK = 16, 64          # the envelope of fk_beam_select / fk_beam_topk


def inv_lenpow_table(n: int, alpha: float) -> Tensor:
    """fp32 [n] on the host: entry L = 1 / L^alpha computed in float64 and rounded once, entry 0 = 1 (the length penalty the beam kernels
    multiply by; alpha = 0 gives ones)."""
    L = torch.arange(max(int(n), 1), dtype=torch.float64)
    L[0] = 1.0
    return (1.0 / L.pow(float(alpha))).to(torch.float32)


class BeamState:
    """Device-side state of a cached beam search of `groups` sentences x `width` beams (row g * width + b): one Philox seed per sentence,
    step counter (= row of the logs the next step writes), cumulative scores [groups * width], the per-step logs parent_log / tok_log
    [steps, groups * width] the host backtracks through (parents are beam numbers inside the sentence), the ancestry table anc
    [groups * width, tmax] (anc[r, j] = the cache slot, counted from the sentence's first, that holds row r's key/value row j) and the
    ticket word of beam_select_grouped.  seed: an int (groups = 1) or a sequence of `groups` ints.
    With eos (an end-of-text id) or a length_penalty alpha != 0 it also holds the state of beam_select_eos / beam_backtrack: fin and len
    [groups * width] int32, inv_lenpow fp32 [steps + 2] (inv_lenpow_table), live_acc and live [1]; otherwise none of these exist."""

    def __init__(self, device, width: int, steps: int, tmax: int, seed=None, groups: int = 1, eos: Optional[int] = None,
                 length_penalty: float = 0.0):
        if seed is None:                                   # follows torch.manual_seed like torch.multinomial would
            seed = torch.randint(0, 2 ** 62, (groups,)).tolist()
        seed = [int(x) for x in seed] if hasattr(seed, "__iter__") else [int(seed)]
        assert len(seed) == groups, f"{groups} sentences need {groups} seeds, got {len(seed)}"
        seed = [x - (1 << 64) if x >= (1 << 63) else x for x in seed]          # 64 raw bits in an int64 tensor
        self.width, self.groups = width, groups
        self.seed = torch.tensor(seed, dtype=torch.int64, device=device)
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.scores = torch.zeros(groups * width, dtype=torch.float32, device=device)
        self.parent_log = torch.empty((max(steps, 1), groups * width), dtype=torch.int32, device=device)
        self.tok_log = torch.empty((max(steps, 1), groups * width), dtype=torch.int64, device=device)
        self.anc = torch.empty((groups * width, tmax), dtype=torch.int32, device=device)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)
        if eos is not None or length_penalty != 0.0:
            self.eos, self.length_penalty = eos, float(length_penalty)
            self.fin = torch.zeros(groups * width, dtype=torch.int32, device=device)
            self.len = torch.zeros(groups * width, dtype=torch.int32, device=device)
            self.inv_lenpow = inv_lenpow_table(max(steps, 1) + 2, length_penalty).to(device)
            self.live_acc = torch.zeros(1, dtype=torch.int32, device=device)
            self.live = torch.full((1,), groups * width, dtype=torch.int32, device=device)


def attn_decode_beam(qkv: Tensor, kv: Tensor, anc: Tensor, pos: Tensor, n_head: int) -> Tensor:
    """one causal query per beam against the rows 0..pos[0] of ITS history: row j < pos[0] is read from the cache slot anc[b, j], the
    row pos[0] from slot b.  qkv [W, 3d] (q = qkv[:, :d]), kv [W, Tmax, 2d], anc int32 [W, >= pos] -> o [W, d]."""
    W, d3 = qkv.shape
    d = d3 // 3
    D = d // n_head
    assert kv.dtype == qkv.dtype and kv.shape[0] == W and kv.shape[2] == 2 * d and kv.stride(2) == 1 and qkv.stride(1) == 1
    assert anc.dtype == torch.int32 and anc.dim() == 2 and anc.shape[0] == W and anc.stride(1) == 1
    assert pos.dtype == torch.int32 and pos.numel() == 1
    out = torch.empty((W, d), dtype=qkv.dtype, device=qkv.device)
    call("fk_attn_decode_beam", qkv.data_ptr(), qkv.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), anc.data_ptr(), anc.stride(0),
         out.data_ptr(), d, pos.data_ptr(), W, n_head, D, 1.0 / math.sqrt(D), fk_dtype(qkv), _stream())
    return out


def beam_topk(logits: Tensor, temperature: float, k: int, top_lp: Optional[Tensor] = None, top_id: Optional[Tensor] = None):
    """log_softmax(logits / temperature) and its k largest entries per row, descending, equal values by ascending id — one launch.
    logits fp32 [R, V] (row stride >= V) -> top_lp fp32 [R, k], top_id int64 [R, k]."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    R, V = logits.shape
    if top_lp is None:
        top_lp = torch.empty((R, k), dtype=torch.float32, device=logits.device)
    if top_id is None:
        top_id = torch.empty((R, k), dtype=torch.int64, device=logits.device)
    assert top_lp.dtype == torch.float32 and top_id.dtype == torch.int64 and top_lp.is_contiguous() and top_id.is_contiguous()
    assert tuple(top_lp.shape) == (R, k) and tuple(top_id.shape) == (R, k)
    call("fk_beam_topk", logits.data_ptr(), logits.stride(0), R, V, float(temperature), int(k), top_lp.data_ptr(), top_id.data_ptr(), _stream())
    return top_lp, top_id


def _beam_select_call(fn: str, S: Optional[int], top_lp: Tensor, top_id: Tensor, state: BeamState, cur: Tensor, pos: Tensor,
                      pos_inc: Optional[Tensor], broadcast: bool, *tail) -> Tensor:
    """The body of beam_select (S = None: one block, rows [W, k] or any [R >= 1, k] with broadcast) and of beam_select_grouped /
    beam_select_eos (S sentences, rows [S * W, k] or [S, k] with broadcast): the asserts and the call of `fn`; `tail` = its arguments
    behind anc_ld."""
    W, k = state.width, top_lp.shape[1]
    assert top_lp.dtype == torch.float32 and top_id.dtype == torch.int64 and top_lp.is_contiguous() and top_id.is_contiguous()
    if S is None:
        assert top_lp.shape == top_id.shape and (broadcast or top_lp.shape[0] == W)
        shape = (W, k)
    else:
        assert top_lp.shape == top_id.shape and top_lp.shape[0] == (S if broadcast else S * W)
        shape = (k if broadcast else W * k, S, W, k)            # the stride between two sentences' rows, in front
    assert cur.dtype == torch.int64 and cur.is_contiguous() and cur.numel() == (S or 1) * W
    assert pos.dtype == torch.int32 and pos.numel() == 1 and (pos_inc is None or (pos_inc.dtype == torch.int32 and pos_inc.numel() == 1))
    call(fn, top_lp.data_ptr(), top_id.data_ptr(), 0 if broadcast else k, *shape, state.scores.data_ptr(), state.seed.data_ptr(),
         state.step.data_ptr(), pos.data_ptr(), _ptr(pos_inc), cur.data_ptr(), state.parent_log.data_ptr(), state.tok_log.data_ptr(),
         state.parent_log.shape[0], state.anc.data_ptr(), state.anc.stride(0), *tail, _stream())
    return cur


def beam_select(top_lp: Tensor, top_id: Tensor, state: BeamState, cur: Tensor, pos: Tensor, pos_inc: Optional[Tensor] = None,
                broadcast: bool = False) -> Tensor:
    """One beam-search step on the device (draw without replacement, keep the W best of W * W, logs, ancestry; see fk_beam_select in
    include/franken_hip.h).  top_lp / top_id [R, k] from beam_topk, R = W, or any R >= 1 with broadcast=True (every beam reads row 0:
    the first step, where all beams are one sequence).  Writes cur [W] int64 (returned) and state; pos int32 [1] is the row the step
    has just appended (negative: leave the ancestry alone); pos_inc (may be pos) is advanced by one."""
    return _beam_select_call("fk_beam_select", None, top_lp, top_id, state, cur, pos, pos_inc, broadcast)


def attn_decode_beam_grouped(qkv: Tensor, kv: Tensor, anc: Tensor, pos: Tensor, n_head: int, groups: int, append: bool = False) -> Tensor:
    """attn_decode_beam for `groups` sentences x W beams: qkv [groups * W, 3d], kv [groups * W, Tmax, 2d], anc int32 [groups * W, >= pos]
    of slots counted from the sentence's first (clamped into [0, W)) -> o [groups * W, d].  append=True also writes qkv[:, d:] to
    kv[:, pos[0]] (kv_append_ folded into this launch) and uses it as the newest row."""
    R, d3 = qkv.shape
    d = d3 // 3
    D = d // n_head
    assert groups >= 1 and R % groups == 0
    assert kv.dtype == qkv.dtype and kv.shape[0] == R and kv.shape[2] == 2 * d and kv.stride(2) == 1 and qkv.stride(1) == 1
    assert anc.dtype == torch.int32 and anc.dim() == 2 and anc.shape[0] == R and anc.stride(1) == 1
    assert pos.dtype == torch.int32 and pos.numel() == 1
    out = torch.empty((R, d), dtype=qkv.dtype, device=qkv.device)
    call("fk_attn_decode_beam_grouped", qkv.data_ptr(), qkv.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), kv.shape[1], anc.data_ptr(),
         anc.stride(0), out.data_ptr(), d, pos.data_ptr(), groups, R // groups, n_head, D, 1.0 / math.sqrt(D), int(bool(append)), fk_dtype(qkv),
         _stream())
    return out


def beam_select_grouped(top_lp: Tensor, top_id: Tensor, state: BeamState, cur: Tensor, pos: Tensor, pos_inc: Optional[Tensor] = None,
                        broadcast: bool = False) -> Tensor:
    """beam_select for state.groups sentences in one launch, one block each (fk_beam_select_grouped).  top_lp / top_id [groups * W, k]
    from beam_topk, or [groups, k] with broadcast=True (every beam of a sentence reads that sentence's row: the first step).  Writes cur
    [groups * W] int64 (returned) and state; the one step counter and pos_inc advance once, by the last block to finish."""
    return _beam_select_call("fk_beam_select_grouped", state.groups, top_lp, top_id, state, cur, pos, pos_inc, broadcast, state.ticket.data_ptr())


def beam_select_eos(top_lp: Tensor, top_id: Tensor, state: BeamState, cur: Tensor, pos: Tensor, pos_inc: Optional[Tensor] = None,
                    broadcast: bool = False) -> Tensor:
    """beam_select_grouped with the end-of-text rules (fk_beam_select_eos; state built with eos= / length_penalty=): a finished beam proposes
    itself once, with its score and its length, the survivors are the W best by score * inv_lenpow[length], state.fin / state.len follow
    them and state.live[0] = the unfinished beams of all sentences after the step.  state.groups = 1 is the one-sentence search."""
    return _beam_select_call("fk_beam_select_eos", state.groups, top_lp, top_id, state, cur, pos, pos_inc, broadcast, state.ticket.data_ptr(),
                             -1 if state.eos is None else int(state.eos), state.fin.data_ptr(), state.len.data_ptr(), state.inv_lenpow.data_ptr(),
                             state.inv_lenpow.numel(), state.live_acc.data_ptr(), state.live.data_ptr())


def beam_backtrack(state: BeamState, out_ids: Tensor, t0: int, pad: int):
    """The walk through state's logs on the device (fk_beam_backtrack).  out_ids int64 [groups, width, cols] (last stride 1, rows dense
    or padded) whose columns < t0 the caller has filled with the prompt: beam `rank` of a sentence (0 = the best by score *
    inv_lenpow[len]) gets its tokens in the columns t0 .. t0 + n - 1, n = min(state.step, rows of the logs), and `pad` behind them.
    -> (out_scores fp32 [groups, width] raw, out_len int32 [groups, width]), ordered like out_ids."""
    S, W = state.groups, state.width
    assert out_ids.dtype == torch.int64 and out_ids.dim() == 3 and tuple(out_ids.shape[:2]) == (S, W) and out_ids.stride(2) == 1
    assert out_ids.stride(0) == W * out_ids.stride(1)
    out_scores = torch.empty((S, W), dtype=torch.float32, device=out_ids.device)
    out_len = torch.empty((S, W), dtype=torch.int32, device=out_ids.device)
    call("fk_beam_backtrack", state.parent_log.data_ptr(), state.tok_log.data_ptr(), state.parent_log.shape[0], S, W, state.step.data_ptr(),
         state.scores.data_ptr(), state.len.data_ptr(), state.inv_lenpow.data_ptr(), state.inv_lenpow.numel(), out_ids.data_ptr(),
         out_ids.stride(1), out_ids.shape[2], int(t0), int(pad), out_scores.data_ptr(), out_len.data_ptr(), _stream())
    return out_scores, out_len


# ------------------------------------------------------------------------------------------- conv (VQ-VAE tokenizer)
def im2col1d(x: Tensor, ksize: int, stride: int = 1, dil: int = 1) -> Tensor:
    """x [B, T, C] -> cols [B * Tout, ksize * C] with the causal left padding dil * (ksize - 1); Tout = (T - 1) // stride + 1."""
    assert x.dim() == 3 and x.is_contiguous()
    B, T, C = x.shape
    tout = (T - 1) // stride + 1
    cols = torch.empty((B * tout, ksize * C), dtype=x.dtype, device=x.device)
    call("fk_im2col1d", x.data_ptr(), cols.data_ptr(), B, T, C, ksize, stride, dil, fk_dtype(x), _stream())
    return cols


def col2im1d(dcols: Tensor, B: int, T: int, C: int, ksize: int, stride: int = 1, dil: int = 1) -> Tensor:
    tout = (T - 1) // stride + 1
    assert dcols.is_contiguous() and dcols.shape == (B * tout, ksize * C)
    dx = torch.empty((B, T, C), dtype=dcols.dtype, device=dcols.device)
    call("fk_col2im1d", dcols.data_ptr(), dx.data_ptr(), B, T, C, ksize, stride, dil, fk_dtype(dcols), _stream())
    return dx


def elu_fwd(x: Tensor) -> Tensor:
    assert x.is_contiguous()
    y = torch.empty_like(x)
    call("fk_elu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), fk_dtype(x), _stream())
    return y


def elu_bwd(x: Tensor, dy: Tensor) -> Tensor:
    assert x.is_contiguous() and dy.is_contiguous() and dy.dtype == x.dtype and dy.shape == x.shape
    dx = torch.empty_like(x)
    call("fk_elu_bwd", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), fk_dtype(x), _stream())
    return dx


def argmax_rows(x: Tensor) -> Tensor:
    assert x.dim() == 2 and x.stride(1) == 1
    idx = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    call("fk_argmax_rows", x.data_ptr(), x.stride(0), idx.data_ptr(), x.shape[0], x.shape[1], fk_dtype(x), _stream())
    return idx


# ------------------------------------------------------------------------------------------- vector quantiser (csrc/vq.hip)
VQ_EMA, VQ_KMEANS = _lib.VQ_EMA, _lib.VQ_KMEANS
_vq_tickets = {}          # device index -> the uint32 word fk_vq_assign's last workgroup is found with (0 between launches)


def vq_route(D: int, K: int, dtype=torch.float32) -> bool:
    """True when vq_assign takes a [*, D] problem with K codes in this dtype (fk_vq_route; host-side query, no launch); a dtype the
    library does not know is outside the envelope like any other."""
    code = {torch.float32: FK_F32, torch.bfloat16: FK_BF16}.get(dtype, -1)
    return lib().fk_vq_route(D, K, code) == _lib.VQ_FUSED


def vq_stats(K: int, D: int, device) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (packed, counts, sums): one cleared fp32 [K, D + 1] tensor and its views sums = packed[:, :D], counts = packed[:, D] — what
    vq_assign accumulates into, vq_codebook_update reads and data parallel all-reduces as ONE tensor."""
    packed = torch.zeros((K, D + 1), dtype=torch.float32, device=device)
    return packed, packed[:, D], packed[:, :D]


def vq_assign(x: Tensor, codes: Tensor, want_q: bool = True, counts: Optional[Tensor] = None, sums: Optional[Tensor] = None,
              commit_scale: Optional[float] = None):
    """Nearest code of every row in one launch: x [R, D] (fp32 / bf16, any row stride), codes fp32 [K, D] -> (idx int64 [R], q [R, D] in
    x's dtype or None, commit fp32 [1] = commit_scale * sum (x - q)^2 or None).  counts [K] / sums [K, D] (fp32 views, see vq_stats) are
    accumulated into when given."""
    assert x.dim() == 2 and x.stride(1) == 1 and codes.dim() == 2 and codes.dtype == torch.float32 and codes.is_contiguous()
    R, D = x.shape
    Kc = codes.shape[0]
    assert codes.shape[1] == D and R > 0
    idx = torch.empty(R, dtype=torch.int64, device=x.device)
    q = torch.empty((R, D), dtype=x.dtype, device=x.device) if want_q else None
    if counts is not None:
        assert counts.dtype == torch.float32 and counts.shape == (Kc,)
    if sums is not None:
        assert sums.dtype == torch.float32 and sums.shape == (Kc, D) and sums.stride(1) == 1
    partials = commit = ticket = None
    if commit_scale is not None:
        partials = torch.empty((R + _lib.VQ_ROWS - 1) // _lib.VQ_ROWS, dtype=torch.float32, device=x.device)
        commit = torch.empty(1, dtype=torch.float32, device=x.device)
        ticket = _vq_tickets.get(x.device.index)
        if ticket is None:
            ticket = _vq_tickets[x.device.index] = torch.zeros(1, dtype=torch.int32, device=x.device)
    with _timed("vq_assign"):
        call("fk_vq_assign", x.data_ptr(), x.stride(0), codes.data_ptr(), idx.data_ptr(), _ptr(q), _ptr(counts),
             counts.stride(0) if counts is not None else 0, _ptr(sums), sums.stride(0) if sums is not None else 0, _ptr(partials),
             _ptr(commit), commit_scale or 0.0, _ptr(ticket), R, Kc, D, fk_dtype(x), _stream())
    return idx, q, commit


def vq_bwd(x: Tensor, q: Tensor, dq: Optional[Tensor], d_commit: Optional[Tensor], c_scale: float) -> Tensor:
    """dx = dq + d_commit * c_scale * (x - q)  (contiguous tensors of one dtype; d_commit a one-element fp32 device tensor)."""
    assert x.is_contiguous() and q.is_contiguous() and q.shape == x.shape and q.dtype == x.dtype
    assert dq is None or (dq.is_contiguous() and dq.shape == x.shape and dq.dtype == x.dtype)
    assert d_commit is None or (d_commit.dtype == torch.float32 and d_commit.numel() == 1)
    dx = torch.empty_like(x)
    with _timed("vq_bwd"):
        call("fk_vq_bwd", x.data_ptr(), q.data_ptr(), _ptr(dq), _ptr(d_commit), c_scale, dx.data_ptr(), x.numel(), fk_dtype(x), _stream())
    return dx


def vq_codebook_update(embed: Tensor, counts: Tensor, sums: Tensor, mode: int, embed_avg: Optional[Tensor] = None,
                       cluster_size: Optional[Tensor] = None, seed: Optional[Tensor] = None, decay: float = 0.0, eps: float = 0.0,
                       dead: float = 0.0) -> Tensor:
    """In place over the K codes (fp32): VQ_EMA — the EMA step with dead-code re-seeding from `seed` [K, D]; VQ_KMEANS — embed_j =
    normalize(sums_j / counts_j) where counts_j > 0 (include/franken_hip.h, fk_vq_codebook_update)."""
    Kc, D = embed.shape
    assert embed.dtype == torch.float32 and embed.is_contiguous()
    assert counts.dtype == torch.float32 and counts.shape == (Kc,) and sums.dtype == torch.float32 and sums.shape == (Kc, D) and sums.stride(1) == 1
    for t, shape in ((embed_avg, (Kc, D)), (cluster_size, (Kc,)), (seed, (Kc, D))):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape)
    n_ws = torch.empty(1, dtype=torch.float32, device=embed.device) if mode == VQ_EMA else None
    with _timed("vq_codebook_update"):
        call("fk_vq_codebook_update", embed.data_ptr(), _ptr(embed_avg), _ptr(cluster_size), counts.data_ptr(), counts.stride(0),
             sums.data_ptr(), sums.stride(0), _ptr(seed), _ptr(n_ws), Kc, D, decay, eps, dead, mode, _stream())
    return embed


# ------------------------------------------------------------------------------------------- losses
def l1_loss_fwd(pred: Tensor, target: Tensor, squared: bool = False, row_weight: Optional[Tensor] = None) -> Tensor:
    """-> loss2 fp32[2] = {mean (weighted) |d| or d^2, weight sum}; row_weight: fp32 [rows] with rows = numel / last dim."""
    assert pred.is_contiguous() and target.is_contiguous() and pred.shape == target.shape and pred.dtype == target.dtype
    loss2 = torch.empty(2, dtype=torch.float32, device=pred.device)
    row_len = pred.shape[-1]
    if row_weight is not None:
        assert row_weight.dtype == torch.float32 and row_weight.is_contiguous() and row_weight.numel() * row_len == pred.numel()
    ws, nb = _ws(lib().fk_loss_workspace_bytes(pred.numel()), pred.device)
    call("fk_l1_loss_fwd", pred.data_ptr(), target.data_ptr(), loss2.data_ptr(), pred.numel(), int(squared), _ptr(row_weight),
         row_len, fk_dtype(pred), _ptr(ws), nb, _stream())
    return loss2


def l1_loss_bwd(pred: Tensor, target: Tensor, gout: Tensor, squared: bool = False, row_weight: Optional[Tensor] = None,
                loss2: Optional[Tensor] = None) -> Tensor:
    assert gout.dtype == torch.float32 and gout.numel() == 1
    d = torch.empty_like(pred)
    call("fk_l1_loss_bwd", pred.data_ptr(), target.data_ptr(), gout.data_ptr(), d.data_ptr(), pred.numel(), int(squared),
         _ptr(row_weight), pred.shape[-1], _ptr(loss2), fk_dtype(pred), _stream())
    return d


def ce_loss_fwd(logits: Tensor, targets: Tensor, ignore_index: int = -100):
    """logits [rows, V] (row stride ok), targets int64 [rows] -> (loss2 fp32[2] = {mean nll, count}, row_lse)."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and targets.dtype == torch.int64 and targets.is_contiguous()
    rows, V = logits.shape
    assert targets.numel() == rows
    loss2 = torch.empty(2, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    ws, nb = _ws(lib().fk_ce_workspace_bytes(rows), logits.device)
    call("fk_ce_loss_fwd", logits.data_ptr(), logits.stride(0), targets.data_ptr(), loss2.data_ptr(), lse.data_ptr(),
         rows, V, ignore_index, fk_dtype(logits), _ptr(ws), nb, _stream())
    return loss2, lse


def ce_loss_bwd(logits: Tensor, targets: Tensor, lse: Tensor, loss2: Tensor, gout: Tensor, dlogits: Tensor,
                ignore_index: int = -100) -> Tensor:
    rows, V = logits.shape
    assert dlogits.shape == logits.shape and dlogits.stride(1) == 1 and dlogits.dtype == logits.dtype
    call("fk_ce_loss_bwd", logits.data_ptr(), logits.stride(0), targets.data_ptr(), lse.data_ptr(), loss2.data_ptr(),
         gout.data_ptr(), dlogits.data_ptr(), dlogits.stride(0), rows, V, ignore_index, fk_dtype(logits), _stream())
    return dlogits


# ------------------------------------------------------------------------------------------- CTC (csrc/ctc.hip)
CTC_ROUTE_NAMES = {_lib.CTC_WAVE: "CTC_WAVE", _lib.CTC_LDS: "CTC_LDS"}
CTC_REDUCTIONS = {"none": _lib.CTC_NONE, "sum": _lib.CTC_SUM, "mean": _lib.CTC_MEAN}


def ctc_route(Lmax: int) -> int:
    """The lattice kernel a target width takes (fk_ctc_route; host-side query, no launch): CTC_WAVE up to 31 labels, CTC_LDS up to 255;
    raises beyond."""
    rc = lib().fk_ctc_route(Lmax)
    _lib.check(0 if rc >= 0 else rc, "fk_ctc_route")
    return rc


class CtcState:
    """What one forward leaves for the backward (and for tests): nll [B] and loss2 = {reduced loss, B}, row_lse [B, T], the workspace and,
    with the lattice, alpha / beta as fp32 [B, T, S_pad] views into it."""
    __slots__ = ("nll", "loss2", "row_lse", "ws", "ws_bytes", "alpha", "beta", "shape", "blank", "reduction", "zero_infinity")


def _ctc_lengths(t: Optional[Tensor], B: int, device) -> Optional[Tensor]:
    if t is None:
        return None
    assert t.dtype == torch.int64 and t.shape == (B,) and t.device == device
    return t.contiguous()


def ctc_loss_fwd(logits: Tensor, targets: Tensor, input_lengths: Optional[Tensor] = None, target_lengths: Optional[Tensor] = None,
                 blank: int = 0, reduction: str = "mean", zero_infinity: bool = False, pad_value: int = -100, want_grad: bool = True,
                 want_lattice: bool = False) -> CtcState:
    """logits [B, T, C] (fp32 / bf16, unit column stride, any row and batch stride), targets int64 [B, Lmax] (unit column stride) ->
    CtcState.  want_grad runs the beta recursion beside the alpha recursion and keeps both lattices for ctc_loss_bwd; want_lattice also
    exposes them (state.alpha, state.beta; tests)."""
    assert logits.dim() == 3 and logits.stride(2) == 1 and targets.dim() == 2 and targets.dtype == torch.int64
    B, T, Cn = logits.shape
    Lmax = targets.shape[1]
    assert targets.shape[0] == B and (Lmax == 0 or targets.stride(1) == 1)
    lattice = want_grad or want_lattice
    st = CtcState()
    dev = logits.device
    st.nll = torch.empty(B, dtype=torch.float32, device=dev)
    st.loss2 = torch.empty(2, dtype=torch.float32, device=dev)
    st.row_lse = torch.empty((B, T), dtype=torch.float32, device=dev)
    st.ws_bytes = lib().fk_ctc_workspace_bytes(B, T if lattice else 0, Lmax)
    st.ws, _ = _ws(st.ws_bytes, dev)
    st.shape, st.blank, st.reduction, st.zero_infinity = (B, T, Cn, Lmax), blank, CTC_REDUCTIONS[reduction], bool(zero_infinity)
    il, tl = _ctc_lengths(input_lengths, B, dev), _ctc_lengths(target_lengths, B, dev)
    with _timed("ctc_loss_fwd"):
        call("fk_ctc_loss_fwd", logits.data_ptr(), logits.stride(0), logits.stride(1), targets.data_ptr() if Lmax else None,
             targets.stride(0) if Lmax else 0, _ptr(il), _ptr(tl), pad_value, st.nll.data_ptr(), st.loss2.data_ptr(), st.row_lse.data_ptr(),
             B, T, Cn, Lmax, blank, st.reduction, int(st.zero_infinity), int(lattice), fk_dtype(logits), _ptr(st.ws), st.ws_bytes, _stream())
    st.alpha = st.beta = None
    if want_lattice:
        s_pad = (2 * Lmax + 1 + 63) // 64 * 64
        n = B * T * s_pad
        lat = st.ws[st.ws_bytes - 2 * _ctc_a256(4 * n):].view(torch.float32)
        st.alpha, st.beta = lat[:n].view(B, T, s_pad), lat[_ctc_a256(4 * n) // 4:][:n].view(B, T, s_pad)
    return st


def _ctc_a256(nbytes: int) -> int:
    return (nbytes + 255) // 256 * 256


def ctc_loss_bwd(logits: Tensor, st: CtcState, gout: Tensor, dlogits: Optional[Tensor] = None) -> Tensor:
    """dlogits (logits' dtype) from the state of a forward that ran with want_grad; gout: fp32 device tensor, one element for 'sum' /
    'mean', [B] for 'none' (the reduction's own factor is applied by the kernel)."""
    B, T, Cn, Lmax = st.shape
    assert tuple(logits.shape) == (B, T, Cn) and logits.stride(2) == 1
    assert gout.dtype == torch.float32 and gout.is_contiguous() and gout.numel() == (B if st.reduction == _lib.CTC_NONE else 1)
    if dlogits is None:
        dlogits = torch.empty((B, T, Cn), dtype=logits.dtype, device=logits.device)
    assert dlogits.shape == logits.shape and dlogits.stride(2) == 1 and dlogits.dtype == logits.dtype
    with _timed("ctc_loss_bwd"):
        call("fk_ctc_loss_bwd", logits.data_ptr(), logits.stride(0), logits.stride(1), st.row_lse.data_ptr(), gout.data_ptr(),
             dlogits.data_ptr(), dlogits.stride(0), dlogits.stride(1), B, T, Cn, Lmax, st.blank, st.reduction, int(st.zero_infinity),
             fk_dtype(logits), st.ws.data_ptr(), st.ws_bytes, _stream())
    return dlogits


def ctc_collapse(argmax: Tensor, input_lengths: Optional[Tensor] = None, blank: int = 0, pad: int = -100) -> Tuple[Tensor, Tensor]:
    """Per-frame argmax int64 [B, T] -> (ids int64 [B, T] padded with `pad`, lengths int64 [B]): repeats merged, blanks dropped."""
    assert argmax.dim() == 2 and argmax.dtype == torch.int64 and argmax.stride(1) == 1
    B, T = argmax.shape
    il = _ctc_lengths(input_lengths, B, argmax.device)
    ids = torch.empty((B, T), dtype=torch.int64, device=argmax.device)
    lengths = torch.empty(B, dtype=torch.int64, device=argmax.device)
    call("fk_ctc_collapse", argmax.data_ptr(), argmax.stride(0), _ptr(il), ids.data_ptr(), ids.stride(0), lengths.data_ptr(), B, T, blank, pad,
         _stream())
    return ids, lengths


CTC_ALIGN_PACK, CTC_ALIGN_CHUNK = 16, 256       # csrc/ctc.hip: frames per back-pointer dword, frames per backtrack chunk in LDS


def ctc_align(logits: Tensor, targets: Tensor, input_lengths: Optional[Tensor] = None, target_lengths: Optional[Tensor] = None, blank: int = 0,
              pad_value: int = -100, pad: int = -100, want_index: bool = True, want_spans: bool = True, out: Optional[dict] = None) -> dict:
    """Forced alignment (fk_ctc_align; semantics: include/franken_hip.h): logits [B, T, C] (fp32 / bf16, unit column stride, any row and
    batch stride, NOT log-softmaxed), targets int64 [B, Lmax] (unit column stride), lengths as ctc_loss_fwd -> dict(score fp32 [B], path
    int64 [B, T], index int64 [B, T], start / end int64 [B, Lmax], label_lp fp32 [B, Lmax]).  want_index / want_spans False: those
    outputs are not computed (None).  out: tensors to write into, by the same names (unit column stride; tests: padded row strides)."""
    assert logits.dim() == 3 and logits.stride(2) == 1 and targets.dim() == 2 and targets.dtype == torch.int64
    B, T, Cn = logits.shape
    Lmax = targets.shape[1]
    assert targets.shape[0] == B and (Lmax == 0 or targets.stride(1) == 1)
    dev = logits.device
    out = dict(out or {})
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    r = {"score": out.get("score", None), "path": out.get("path", None), "index": None, "start": None, "end": None, "label_lp": None}
    if r["score"] is None:
        r["score"] = new((B,), torch.float32)
    if r["path"] is None:
        r["path"] = new((B, T), torch.int64)
    if want_index:
        r["index"] = out["index"] if "index" in out else new((B, T), torch.int64)
    if want_spans:
        for k, dt in (("start", torch.int64), ("end", torch.int64), ("label_lp", torch.float32)):
            r[k] = out[k] if k in out else new((B, Lmax), dt)
    assert r["score"].dtype == torch.float32 and r["score"].shape == (B,) and r["score"].is_contiguous()
    for k, n, dt in (("path", T, torch.int64), ("index", T, torch.int64), ("start", Lmax, torch.int64), ("end", Lmax, torch.int64),
                     ("label_lp", Lmax, torch.float32)):
        t = r[k]
        assert t is None or (t.dtype == dt and t.shape == (B, n) and (n == 0 or t.stride(1) == 1)), k
    ld_lab = {r[k].stride(0) for k in ("start", "end", "label_lp") if r[k] is not None}
    assert len(ld_lab) <= 1, "start, end and label_lp share one row stride"
    nbytes = lib().fk_ctc_align_workspace_bytes(B, T, Lmax)
    ws, _ = _ws(nbytes, dev)
    il, tl = _ctc_lengths(input_lengths, B, dev), _ctc_lengths(target_lengths, B, dev)
    with _timed("ctc_align"):
        call("fk_ctc_align", logits.data_ptr(), logits.stride(0), logits.stride(1), targets.data_ptr() if Lmax else None,
             targets.stride(0) if Lmax else 0, _ptr(il), _ptr(tl), pad_value, B, T, Cn, Lmax, blank, pad, r["score"].data_ptr(),
             r["path"].data_ptr(), r["path"].stride(0), _ptr(r["index"]), r["index"].stride(0) if want_index else 0, _ptr(r["start"]),
             _ptr(r["end"]), _ptr(r["label_lp"]), ld_lab.pop() if ld_lab else 0, fk_dtype(logits), _ptr(ws), nbytes, _stream())
    return r


def _ctc_beam_prologue(logits: Tensor, input_lengths: Optional[Tensor], beam_width: int, topk: Optional[int], nbest: int,
                       ws_bytes: str = "fk_ctc_beam_workspace_bytes"):
    """What the beam searches set up before their call -> (B, T, C, K, il, ids, lengths, ws, nbytes); topk None: min(32, C - 1)."""
    assert logits.dim() == 3 and logits.stride(2) == 1 and logits.dtype in (torch.float32, torch.bfloat16)
    B, T, Cn = logits.shape
    K = min(32, Cn - 1) if topk is None else int(topk)
    dev = logits.device
    il = _ctc_lengths(input_lengths, B, dev)
    ids = torch.empty((B, nbest, T), dtype=torch.int64, device=dev)
    lengths = torch.empty((B, nbest), dtype=torch.int64, device=dev)
    nbytes = getattr(lib(), ws_bytes)(B, T, beam_width, K)
    ws, _ = _ws(nbytes, dev)
    return B, T, Cn, K, il, ids, lengths, ws, nbytes


def ctc_beam_search(logits: Tensor, input_lengths: Optional[Tensor] = None, blank: int = 0, beam_width: int = 8, topk: Optional[int] = None,
                    nbest: int = 1, pad: int = -100) -> Tuple[Tensor, Tensor, Tensor]:
    """Prefix beam search over logits [B, T, C] (fp32 / bf16, unit column stride, any row and batch stride; NOT log-softmaxed) ->
    (ids int64 [B, nbest, T] padded with `pad`, lengths int64 [B, nbest], scores fp32 [B, nbest]): the nbest most probable labellings
    the beam found, best first, with their log-probability mass (semantics: include/franken_hip.h).  beam_width and topk (new prefixes
    proposed per resident prefix and frame; None: min(32, C - 1)) up to 32.  A slot without hypothesis: length 0, score -inf."""
    B, T, Cn, K, il, ids, lengths, ws, nbytes = _ctc_beam_prologue(logits, input_lengths, beam_width, topk, nbest)
    scores = torch.empty((B, nbest), dtype=torch.float32, device=logits.device)
    with _timed("ctc_beam_search"):
        call("fk_ctc_beam_search", logits.data_ptr(), logits.stride(0), logits.stride(1), _ptr(il), B, T, Cn, blank, beam_width, K, nbest, pad,
             ids.data_ptr(), ids.stride(0), ids.stride(1), lengths.data_ptr(), scores.data_ptr(), fk_dtype(logits), _ptr(ws), nbytes, _stream())
    return ids, lengths, scores


def ctc_beam_search_lm(logits: Tensor, lm, input_lengths: Optional[Tensor] = None, blank: int = 0, beam_width: int = 8, topk: Optional[int] = None,
                       nbest: int = 1, lm_weight: float = 1.0, length_bonus: float = 0.0, use_eos: bool = True,
                       pad: int = -100) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """ctc_beam_search with the backoff n-gram model `lm` (utils.ngram.NGramLM, or its compile()d tables) inside the selection:
    key = CTC total + lm_weight * ln P_lm + length_bonus * length (semantics: include/franken_hip.h) -> (ids int64 [B, nbest, T], lengths
    int64 [B, nbest], am fp32 [B, nbest] the pure CTC mass, lm fp32 [B, nbest] the unweighted ln P_lm, total fp32 [B, nbest] the final
    key), best first.  The model's n_classes must be C."""
    tables = lm.compile() if hasattr(lm, "compile") else lm
    if tables.n_classes != logits.shape[-1]:
        raise ValueError(f"the language model has {tables.n_classes} classes, the logits {logits.shape[-1]}")
    B, T, Cn, K, il, ids, lengths, ws, nbytes = _ctc_beam_prologue(logits, input_lengths, beam_width, topk, nbest)
    d = tables.to(logits.device)
    am, lms, total = (torch.empty((B, nbest), dtype=torch.float32, device=logits.device) for _ in range(3))
    with _timed("ctc_beam_search_lm"):
        call("fk_ctc_beam_search_lm", logits.data_ptr(), logits.stride(0), logits.stride(1), _ptr(il), B, T, Cn, blank, beam_width, K, nbest, pad,
             d["table"].data_ptr(), tables.cap, tables.max_probe, d["bow"].data_ptr(), d["backoff"].data_ptr(), tables.n_states,
             d["uni_lp"].data_ptr(), d["uni_next"].data_ptr(), tables.start_state, tables.order, float(lm_weight), float(length_bonus),
             int(bool(use_eos)), ids.data_ptr(), ids.stride(0), ids.stride(1), lengths.data_ptr(), am.data_ptr(), lms.data_ptr(),
             total.data_ptr(), fk_dtype(logits), _ptr(ws), nbytes, _stream())
    return ids, lengths, am, lms, total


def ctc_beam_search_lex(logits: Tensor, lexicon, lm=None, sep: int = 1, input_lengths: Optional[Tensor] = None, blank: int = 0, beam_width: int = 8,
                        topk: Optional[int] = None, nbest: int = 1, lm_weight: float = 1.0, word_bonus: float = 0.0, use_eos: bool = True,
                        pad: int = -100):
    """ctc_beam_search constrained to labellings that spell words of `lexicon` (utils.lexicon.Lexicon, or its compile()d tables) separated
    by the class `sep`, with the word-level backoff n-gram model `lm` (utils.ngram.NGramLM over the lexicon's word ids, its tables, or
    None: only word_bonus acts) applied at word ends (semantics: include/franken_hip.h) -> (words int64 [B, nbest, (T + 1) // 2] padded
    with `pad`, word_lengths int64 [B, nbest], ids int64 [B, nbest, T], lengths int64 [B, nbest], am / lm / total fp32 [B, nbest],
    complete uint8 [B, nbest]), best first."""
    lex = lexicon.compile() if hasattr(lexicon, "compile") else lexicon
    tables = lex.null_lm() if lm is None else (lm.compile() if hasattr(lm, "compile") else lm)
    if tables.n_classes != lex.n_words:
        raise ValueError(f"the word model has {tables.n_classes} words, the lexicon {lex.n_words}")
    if blank in lex.classes or sep in lex.classes or max(lex.classes) >= logits.shape[-1]:
        raise ValueError(f"a pronunciation holds the blank {blank}, the separator {sep} or a class outside the head's {logits.shape[-1]}")
    B, T, Cn, K, il, ids, lengths, ws, nbytes = _ctc_beam_prologue(logits, input_lengths, beam_width, topk, nbest, "fk_ctc_beam_lex_workspace_bytes")
    dev = logits.device
    d, t = tables.to(dev), lex.to(dev)
    Lw = (T + 1) // 2
    words = torch.empty((B, nbest, Lw), dtype=torch.int64, device=dev)
    word_lengths = torch.empty((B, nbest), dtype=torch.int64, device=dev)
    complete = torch.empty((B, nbest), dtype=torch.uint8, device=dev)
    am, lms, total = (torch.empty((B, nbest), dtype=torch.float32, device=dev) for _ in range(3))
    with _timed("ctc_beam_search_lex"):
        call("fk_ctc_beam_search_lex", logits.data_ptr(), logits.stride(0), logits.stride(1), _ptr(il), B, T, Cn, blank, sep, beam_width, K, nbest, pad,
             t["table"].data_ptr(), lex.cap, lex.max_probe, t["node_words"].data_ptr(), lex.n_nodes, t["word_list"].data_ptr(),
             int(t["word_list"].numel()), lex.n_words, d["table"].data_ptr(), tables.cap, tables.max_probe, d["bow"].data_ptr(),
             d["backoff"].data_ptr(), tables.n_states, d["uni_lp"].data_ptr(), d["uni_next"].data_ptr(), tables.start_state, tables.order,
             float(lm_weight), float(word_bonus), int(bool(use_eos)), words.data_ptr(), words.stride(0), words.stride(1), word_lengths.data_ptr(),
             ids.data_ptr(), ids.stride(0), ids.stride(1), lengths.data_ptr(), am.data_ptr(), lms.data_ptr(), total.data_ptr(),
             complete.data_ptr(), fk_dtype(logits), _ptr(ws), nbytes, _stream())
    return words, word_lengths, ids, lengths, am, lms, total, complete


# ------------------------------------------------------------------------------------------- joint CTC / attention decoding
CTC_PREFIX_MAX_T, CTC_PREFIX_MAX_PROMPT, CTC_PREFIX_FLOOR = _lib.CTC_PREFIX_MAX_T, _lib.CTC_PREFIX_MAX_PROMPT, _lib.CTC_PREFIX_FLOOR


class CtcPrefixState:
    """Device-side state of the CTC prefix scorer inside a beam search of S sentences x `width` beams (fk_ctc_prefix_* in
    include/franken_hip.h has the rule): the logits [S, T, C] of the frame-synchronous head (kept, not copied), row_lse [S, T], the two
    state buffers st[0] / st[1] fp32 [S * width, 2, T] (r_n, then r_b) that swap by the parity of the step, psi fp32 and last int32
    [2, S * width] whose halves swap with them, the clamped-on-device lengths, the blank and the weight of the CTC term."""
    __slots__ = ("logits", "row_lse", "st", "psi", "last", "lengths", "blank", "weight", "width")


def ctc_prefix_init(logits: Tensor, width: int, weight: float, blank: Optional[int] = None, input_lengths: Optional[Tensor] = None,
                    prompt: Optional[Tensor] = None) -> CtcPrefixState:
    """row_lse and the state of every row of a beam search before its first step: the empty hypothesis, advanced by the labels in
    `prompt` (int64 [S, P], None: none).  logits [S, T, C] fp32 / bf16, unit column stride, any row and batch stride; blank None: C - 1.
    The state buffers come from torch.empty: the kernels write every element before they read it."""
    assert logits.dim() == 3 and logits.stride(2) == 1 and logits.dtype in (torch.float32, torch.bfloat16)
    S, T, Cn = logits.shape
    dev = logits.device
    st = CtcPrefixState()
    st.logits, st.width, st.weight, st.blank = logits, int(width), float(weight), Cn - 1 if blank is None else int(blank)
    st.lengths = _ctc_lengths(input_lengths, S, dev)
    R = S * st.width
    st.row_lse = torch.empty((S, T), dtype=torch.float32, device=dev)
    st.st = (torch.empty((R, 2, T), dtype=torch.float32, device=dev), torch.empty((R, 2, T), dtype=torch.float32, device=dev))
    st.psi = torch.empty((2, R), dtype=torch.float32, device=dev)
    st.last = torch.empty((2, R), dtype=torch.int32, device=dev)
    P = 0
    if prompt is not None:
        assert prompt.dtype == torch.int64 and prompt.dim() == 2 and prompt.shape[0] == S and prompt.device == dev
        prompt = prompt.contiguous()
        P = prompt.shape[1]
    call("fk_ctc_prefix_init", logits.data_ptr(), logits.stride(0), logits.stride(1), _ptr(st.lengths), S, T, Cn, st.blank, st.width,
         _ptr(prompt) if P else None, P, P, st.row_lse.data_ptr(), st.st[0].data_ptr(), st.psi.data_ptr(), st.last.data_ptr(), fk_dtype(logits),
         _stream())
    return st


def ctc_prefix_score_(top_lp: Tensor, top_id: Tensor, state: CtcPrefixState, beam_state: BeamState, broadcast: bool = False) -> Tensor:
    """top_lp <- (1 - weight) * top_lp + weight * (psi(h c) - psi(h)) for the k candidates of every row, in place, one launch between
    beam_topk and beam_select* (fk_ctc_prefix_score).  At beam_state.step > 0 every row's state first follows the parent and the token the
    last select logged; rows of finished beams (beam_state.fin) stay as they are.  top_lp / top_id [S * W, k], or [S, k] with
    broadcast=True (the first step: nothing advances)."""
    S, T, Cn = state.logits.shape
    W, k = state.width, top_lp.shape[1]
    assert beam_state.width == W and beam_state.groups == S
    assert top_lp.dtype == torch.float32 and top_id.dtype == torch.int64 and top_lp.is_contiguous() and top_id.is_contiguous()
    assert top_lp.shape == top_id.shape and top_lp.shape[0] == (S if broadcast else S * W)
    fin = getattr(beam_state, "fin", None)
    eos = getattr(beam_state, "eos", None)
    call("fk_ctc_prefix_score", state.logits.data_ptr(), state.logits.stride(0), state.logits.stride(1), _ptr(state.lengths),
         state.row_lse.data_ptr(), S, T, Cn, state.blank, W, k, top_lp.data_ptr(), top_id.data_ptr(), int(bool(broadcast)), state.weight,
         -1 if eos is None else int(eos), _ptr(fin), beam_state.step.data_ptr(), beam_state.parent_log.data_ptr(), beam_state.tok_log.data_ptr(),
         beam_state.parent_log.shape[0], state.st[0].data_ptr(), state.st[1].data_ptr(), state.psi.data_ptr(), state.last.data_ptr(),
         fk_dtype(state.logits), _stream())
    return top_lp


class CeChunkState:
    """per-row running statistics of the chunked cross entropy (fk_ce_chunk_*)"""

    def __init__(self, rows: int, device):
        self.m = torch.empty(rows, dtype=torch.float32, device=device)
        self.s = torch.empty(rows, dtype=torch.float32, device=device)
        self.t = torch.empty(rows, dtype=torch.float32, device=device)
        self.first = True


def ce_chunk_fwd(logits: Tensor, targets: Tensor, col0: int, st: CeChunkState) -> None:
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1 and targets.dtype == torch.int64 and targets.is_contiguous()
    rows, cw = logits.shape
    call("fk_ce_chunk_fwd", logits.data_ptr(), logits.stride(0), targets.data_ptr(), col0, st.m.data_ptr(), st.s.data_ptr(), st.t.data_ptr(),
         rows, cw, int(st.first), _stream())
    st.first = False


def ce_chunk_finish(st: CeChunkState, targets: Tensor, V: int, ignore_index: int = -100):
    rows = targets.numel()
    loss2 = torch.empty(2, dtype=torch.float32, device=targets.device)
    lse = torch.empty(rows, dtype=torch.float32, device=targets.device)
    ws, nb = _ws(lib().fk_ce_workspace_bytes(rows), targets.device)
    call("fk_ce_chunk_finish", st.m.data_ptr(), st.s.data_ptr(), st.t.data_ptr(), targets.data_ptr(), lse.data_ptr(), loss2.data_ptr(),
         rows, V, ignore_index, _ptr(ws), nb, _stream())
    return loss2, lse


def ce_chunk_bwd(logits: Tensor, targets: Tensor, col0: int, cw_valid: int, lse: Tensor, loss2: Tensor, gout: Tensor, dl: Tensor, V: int,
                 ignore_index: int = -100) -> Tensor:
    rows, cw = dl.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and dl.stride(1) == 1 and logits.shape[0] == rows
    call("fk_ce_chunk_bwd", logits.data_ptr(), logits.stride(0), targets.data_ptr(), col0, lse.data_ptr(), loss2.data_ptr(), gout.data_ptr(),
         dl.data_ptr(), dl.stride(0), rows, cw, cw_valid, V, ignore_index, fk_dtype(dl), _stream())
    return dl


def head_ce_fwd(h: Tensor, w: Tensor, bias: Optional[Tensor], targets: Tensor, V: int, ignore_index: int = -100):
    """(loss2, row_lse) of mean CE(h @ w[:V]^T (+ bias), targets) without the [rows, V] logits (fk_head_ce_fwd + fk_ce_chunk_finish)."""
    assert h.dim() == 2 and w.dim() == 2 and h.shape[1] == w.shape[1] and h.dtype == w.dtype and h.stride(1) == 1 and w.stride(1) == 1
    assert w.shape[0] >= V and targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == h.shape[0]
    rows, Kd = h.shape
    if bias is not None:
        assert bias.dtype == h.dtype and bias.is_contiguous() and bias.numel() >= V
    st = CeChunkState(rows, h.device)
    ws, nb = _ws(lib().fk_head_ce_workspace_bytes(rows, V), h.device)
    with _timed(f"head_ce_fwd:{rows}x{V}x{Kd}"):
        call("fk_head_ce_fwd", h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), w.shape[0], _ptr(bias), targets.data_ptr(),
             st.m.data_ptr(), st.s.data_ptr(), st.t.data_ptr(), rows, V, Kd, fk_dtype(h), _ptr(ws), nb, _stream())
    st.first = False
    return ce_chunk_finish(st, targets, V, ignore_index)


def head_ce_stats(h: Tensor, w: Tensor, bias: Optional[Tensor], targets: Tensor, V: int):
    """The per-row statistics of fk_head_ce_fwd that head_ce_fwd folds into a loss: (row_m, row_s, row_t) fp32 [rows] = running maximum, sum
    of exp(logit - row_m) and target logit of h @ w[:V]^T (+ bias), so that log p(target) = row_t - (row_m + log(row_s)); no [rows, V] logits.
    A target outside [0, V) (-100) leaves row_t = 0."""
    assert h.dim() == 2 and w.dim() == 2 and h.shape[1] == w.shape[1] and h.dtype == w.dtype and h.stride(1) == 1 and w.stride(1) == 1
    assert w.shape[0] >= V and targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == h.shape[0]
    rows, Kd = h.shape
    if bias is not None:
        assert bias.dtype == h.dtype and bias.is_contiguous() and bias.numel() >= V
    st = CeChunkState(rows, h.device)
    ws, nb = _ws(lib().fk_head_ce_workspace_bytes(rows, V), h.device)
    with _timed(f"head_ce_fwd:{rows}x{V}x{Kd}"):
        call("fk_head_ce_fwd", h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), w.shape[0], _ptr(bias), targets.data_ptr(),
             st.m.data_ptr(), st.s.data_ptr(), st.t.data_ptr(), rows, V, Kd, fk_dtype(h), _ptr(ws), nb, _stream())
    return st.m, st.s, st.t


def head_ce_bwd(h: Tensor, w: Tensor, bias: Optional[Tensor], targets: Tensor, lse: Tensor, loss2: Tensor, gout: Tensor, V: int,
                vpad: int, rows_pad: int, want_bias: bool, ignore_index: int = -100):
    """dlT [vpad, rows_pad] (transposed d-logits, zero padded) and, for a head with bias, its gradient [V] (fk_head_ce_bwd)."""
    rows, Kd = h.shape
    dlT = torch.empty((vpad, rows_pad), dtype=h.dtype, device=h.device)
    dbpart = torch.empty((2 * ((rows + 127) // 128), vpad), dtype=torch.float32, device=h.device) if want_bias else None
    with _timed(f"head_ce_bwd:{rows}x{V}x{Kd}"):
        call("fk_head_ce_bwd", h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), w.shape[0], _ptr(bias), targets.data_ptr(),
             lse.data_ptr(), loss2.data_ptr(), gout.data_ptr(), dlT.data_ptr(), dlT.stride(0), rows_pad, vpad, _ptr(dbpart), rows, V, Kd,
             ignore_index, fk_dtype(h), _stream())
    db = colsum(dbpart)[:V] if want_bias else None
    return dlT, db


def transpose2d(src: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out[c, r] = src[r, c]; a given `out` may be larger (its padding is left as it is)."""
    assert src.dim() == 2 and src.stride(1) == 1
    rows, cols = src.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=src.dtype, device=src.device)
    assert out.dtype == src.dtype and out.stride(1) == 1 and out.shape[0] >= cols and out.shape[1] >= rows
    call("fk_transpose2d", src.data_ptr(), src.stride(0), out.data_ptr(), out.stride(0), rows, cols, fk_dtype(src), _stream())
    return out


# ------------------------------------------------------------------------------------------- GPT embedding
def gpt_embed_fwd(idx: Tensor, prefix: Optional[Tensor], wte: Tensor, wpe: Tensor, dtype: torch.dtype) -> Tensor:
    B, t_words = idx.shape
    t_ctx = 0 if prefix is None else prefix.shape[1]
    dim = wte.shape[1]
    assert idx.dtype == torch.int64 and idx.is_contiguous() and wte.dtype == torch.float32 and wpe.dtype == torch.float32
    assert wte.is_contiguous() and wpe.is_contiguous() and wpe.shape[0] >= t_ctx + t_words
    if prefix is not None:
        assert prefix.is_contiguous() and prefix.dtype == dtype and prefix.shape == (B, t_ctx, dim)
    out = torch.empty((B, t_ctx + t_words, dim), dtype=dtype, device=idx.device)
    call("fk_gpt_embed_fwd", idx.data_ptr(), _ptr(prefix), wte.data_ptr(), wpe.data_ptr(), out.data_ptr(), B, t_ctx,
         t_words, dim, wte.shape[0], fk_dtype(dtype), _stream())
    return out


def gpt_embed_pos(tok: Tensor, depth: Tensor, prefix: Optional[Tensor], wte: Tensor, wpe: Tensor, dtype: torch.dtype) -> Tensor:
    """The input rows of a packed n-best forward (fk_gpt_embed_pos): out[b, t] = prefix[b, t] + wpe[t] for t < P, out[b, P + i] =
    wte[tok[b, i]] + wpe[P + depth[b, i]]; tok / depth int32 [B, N] (nbest_trie) -> [B, P + N, dim] in `dtype`.  Inference only."""
    B, N = tok.shape
    P = 0 if prefix is None else prefix.shape[1]
    dim = wte.shape[1]
    assert tok.dtype == torch.int32 and depth.dtype == torch.int32 and tok.is_contiguous() and depth.is_contiguous() and depth.shape == (B, N)
    assert wte.dtype == torch.float32 and wpe.dtype == torch.float32 and wte.is_contiguous() and wpe.is_contiguous() and wpe.shape[1] == dim
    if prefix is not None:
        assert prefix.is_contiguous() and prefix.dtype == dtype and prefix.shape == (B, P, dim)
    out = torch.empty((B, P + N, dim), dtype=dtype, device=tok.device)
    call("fk_gpt_embed_pos", tok.data_ptr(), depth.data_ptr(), _ptr(prefix), wte.data_ptr(), wpe.data_ptr(), out.data_ptr(), B, P, N, dim,
         wte.shape[0], wpe.shape[0], fk_dtype(dtype), _stream())
    return out


def gpt_embed_bwd_wte(idx: Tensor, dout: Tensor, dwte: Tensor, t_ctx: int) -> None:
    B, t_words = idx.shape
    assert dout.is_contiguous() and dwte.dtype == torch.float32 and dwte.is_contiguous()
    call("fk_gpt_embed_bwd_wte", idx.data_ptr(), dout.data_ptr(), dwte.data_ptr(), B, t_ctx, t_words, dwte.shape[1],
         dwte.shape[0], fk_dtype(dout), _stream())


# ------------------------------------------------------------------------------------------- optimizer
def adamw_step_(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: int, lr: float, beta1: float = 0.9,
                beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 1e-2, clip: float = 0.0,
                grad_scale: float = 1.0, zero_grad: bool = False) -> None:
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
    call("fk_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
         weight_decay, step, clip, grad_scale, int(zero_grad), _stream())


ADAMW_MAX_SLOTS, GRAD_SUMSQ_BLOCKS = _lib.ADAMW_MAX_SLOTS, _lib.GRAD_SUMSQ_MAX_BLOCKS


def adamw_segments(segments, device) -> Tensor:
    """The device table of fk_adamw_step_groups / fk_grad_sumsq from [(begin, end, slot)] (element offsets, multiples of 4, sorted by
    begin, disjoint): int64 [nseg, 3], the record layout of fk_adamw_seg (slot in the low half of the third word)."""
    rows = [(int(b), int(e), int(s)) for b, e, s in segments]
    prev = 0
    for b, e, s in rows:
        if b % 4 or e % 4 or not (prev <= b < e) or not (0 <= s < ADAMW_MAX_SLOTS):
            raise ValueError(f"segment ({b}, {e}, {s}): edges must be multiples of 4, segments sorted and disjoint, slot in 0..{ADAMW_MAX_SLOTS - 1}")
        prev = e
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(device)


def _check_segments(g: Tensor, segs: Tensor) -> None:
    assert segs.dtype == torch.int64 and segs.dim() == 2 and segs.shape[1] == 3 and segs.is_contiguous() and segs.device == g.device


def grad_sumsq_(g: Tensor, segs: Tensor, partials: Optional[Tensor] = None) -> Tensor:
    """partials [GRAD_SUMSQ_BLOCKS] fp32 whose sum is sum g^2 over the segments of `segs` (adamw_segments); fixed order, the same
    bits on every run.  adamw_step_groups_(max_norm > 0) adds them up itself."""
    assert g.dtype == torch.float32 and g.is_contiguous()
    _check_segments(g, segs)
    if partials is None:
        partials = torch.empty(GRAD_SUMSQ_BLOCKS, dtype=torch.float32, device=g.device)
    assert partials.dtype == torch.float32 and partials.is_contiguous() and 1 <= partials.numel() <= GRAD_SUMSQ_BLOCKS
    call("fk_grad_sumsq", g.data_ptr(), g.numel(), segs.data_ptr(), segs.shape[0], partials.data_ptr(), partials.numel(), _stream())
    return partials


def adamw_step_groups_(p: Tensor, g: Tensor, m: Tensor, v: Tensor, segs: Tensor, slots, clip: float = 0.0, grad_scale: float = 1.0,
                       zero_grad: bool = False, max_norm: float = 0.0, partials: Optional[Tensor] = None,
                       norm_out: Optional[Tensor] = None) -> None:
    """fk_adamw_step_groups: AdamW over the segments of `segs` (adamw_segments) in one launch; `slots` is a sequence of at most
    ADAMW_MAX_SLOTS (lr, beta1, beta2, eps, weight_decay, step) and a segment's slot picks one.  max_norm > 0: the gradient is
    also scaled by min(1, max_norm / (grad_scale * sqrt(sum(partials)) + 1e-6)) with `partials` from grad_sumsq_ on the same
    gradient, and that norm is stored in norm_out[0]."""
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
    _check_segments(g, segs)
    arr = (_lib.AdamwGroup * max(1, len(slots)))(*[_lib.AdamwGroup(float(lr), float(b1), float(b2), float(eps), float(wd), int(step))
                                                  for lr, b1, b2, eps, wd, step in slots])
    if max_norm > 0:
        assert partials is not None and norm_out is not None and partials.dtype == torch.float32 and norm_out.dtype == torch.float32
        assert partials.is_contiguous() and partials.device == g.device and norm_out.device == g.device and norm_out.numel() >= 1
    call("fk_adamw_step_groups", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), segs.data_ptr(), segs.shape[0],
         arr, len(slots), clip, grad_scale, int(zero_grad), max_norm, _ptr(partials), 0 if partials is None else partials.numel(),
         _ptr(norm_out), _stream())


# ------------------------------------------------------------------------------------------- n-best rescoring (csrc/rescore.hip)
NBEST_MAX_HYPS, NBEST_MAX_T, NBEST_MAX_NODES, NBEST_MAX_ROWS = _lib.NBEST_MAX_HYPS, _lib.NBEST_MAX_T, _lib.NBEST_MAX_NODES, _lib.NBEST_MAX_ROWS


class NbestTrie:
    """what nbest_trie leaves on the device: tok / depth / parent int32 [B, node_cap], leaf int32 [B, n], n_nodes int32 [B] and (heads=True)
    head_src / head_tgt int64 [B, node_cap - 1 + n]; P is the number of prefix rows the head rows count from"""
    __slots__ = ("tok", "depth", "parent", "leaf", "n_nodes", "head_src", "head_tgt", "node_cap", "P")


def _nbest_ids(ids: Tensor, lengths: Tensor, am: Optional[Tensor]):
    assert ids.dim() == 3 and ids.dtype == torch.int64 and ids.stride(2) == 1, "ids: int64 [B, n, T] with unit token stride"
    B, n, T = ids.shape
    assert lengths.dtype == torch.int64 and lengths.shape == (B, n) and lengths.is_contiguous(), "lengths: contiguous int64 [B, n]"
    if am is not None:
        assert am.dtype == torch.float32 and am.shape == (B, n) and am.is_contiguous(), "am: contiguous fp32 [B, n]"
    return B, n, T


def nbest_trie(ids: Tensor, lengths: Tensor, am: Optional[Tensor], V: int, bos: int, eos: Optional[int], node_cap: int, P: int = 0,
               heads: bool = True) -> NbestTrie:
    """The trie of every sentence's n-best list (fk_nbest_trie; semantics: include/franken_hip.h).  ids int64 [B, n, T] (any batch and
    hypothesis stride), lengths int64 [B, n], am fp32 [B, n] or None, eos None: no end-of-text row.  heads=False: the head-row lists are
    not written (a sizing pass that only wants n_nodes)."""
    B, n, T = _nbest_ids(ids, lengths, am)
    dev = ids.device
    t = NbestTrie()
    t.node_cap, t.P = int(node_cap), int(P)
    cap = max(t.node_cap, 1)
    t.tok, t.depth, t.parent = (torch.empty((B, cap), dtype=torch.int32, device=dev) for _ in range(3))
    t.leaf = torch.empty((B, n), dtype=torch.int32, device=dev)
    t.n_nodes = torch.empty(B, dtype=torch.int32, device=dev)
    t.head_src = torch.empty((B, cap - 1 + n), dtype=torch.int64, device=dev) if heads else None
    t.head_tgt = torch.empty((B, cap - 1 + n), dtype=torch.int64, device=dev) if heads else None
    with _timed("nbest_trie"):
        call("fk_nbest_trie", ids.data_ptr(), ids.stride(0), ids.stride(1), lengths.data_ptr(), _ptr(am), B, n, T, V, bos, -1 if eos is None else eos,
             t.node_cap, t.P, t.tok.data_ptr(), t.depth.data_ptr(), t.parent.data_ptr(), t.leaf.data_ptr(), t.n_nodes.data_ptr(), _ptr(t.head_src),
             _ptr(t.head_tgt), _stream())
    return t


def nbest_trie_mask(parent: Tensor, n_nodes: Tensor, P: int) -> Mask:
    """The visibility table of the packed forward as a dense attention mask (fk_nbest_trie_mask): uint8 [B, 1, P + N, P + N]."""
    assert parent.dtype == torch.int32 and parent.dim() == 2 and parent.is_contiguous() and n_nodes.dtype == torch.int32 and n_nodes.is_contiguous()
    B, N = parent.shape
    R = P + N
    table = torch.empty((B, 1, R, R), dtype=torch.uint8, device=parent.device)
    with _timed("nbest_trie_mask"):
        call("fk_nbest_trie_mask", parent.data_ptr(), n_nodes.data_ptr(), table.data_ptr(), B, P, N, _stream())
    return Mask(MASK_DENSE, 0 if B == 1 else R * R, 0, 0, table, None)


def nbest_rescore(stats, trie: NbestTrie, ids: Tensor, lengths: Tensor, am: Optional[Tensor], has_eos: bool, am_weight: float = 1.0,
                  lm_weight: float = 1.0, length_bonus: float = 0.0, pad: int = -100):
    """stats = (row_m, row_s, row_t) of head_ce_stats on the trie's head rows -> (lm fp32 [B, n] in input order, ranked) with ranked =
    (ids [B, n, T] padded with `pad`, lengths, am, lm, total, order int64 [B, n], n_scored int64 [B]) in the new order (fk_nbest_rescore)."""
    B, n, T = _nbest_ids(ids, lengths, am)
    N, dev = trie.node_cap, ids.device
    row_m, row_s, row_t = stats
    for r in stats:
        assert r.dtype == torch.float32 and r.is_contiguous() and r.numel() == B * (N - 1 + n)
    lm = torch.empty((B, n), dtype=torch.float32, device=dev)
    ids_out = torch.empty((B, n, T), dtype=torch.int64, device=dev)
    len_out = torch.empty((B, n), dtype=torch.int64, device=dev)
    am_out, lm_out, total = (torch.empty((B, n), dtype=torch.float32, device=dev) for _ in range(3))
    order = torch.empty((B, n), dtype=torch.int64, device=dev)
    n_scored = torch.empty(B, dtype=torch.int64, device=dev)
    with _timed("nbest_rescore"):
        call("fk_nbest_rescore", row_m.data_ptr(), row_s.data_ptr(), row_t.data_ptr(), trie.depth.data_ptr(), trie.parent.data_ptr(),
             trie.leaf.data_ptr(), trie.n_nodes.data_ptr(), ids.data_ptr(), ids.stride(0), ids.stride(1), lengths.data_ptr(), _ptr(am), B, n, T, N,
             int(has_eos), am_weight, lm_weight, length_bonus, pad, lm.data_ptr(), ids_out.data_ptr(), len_out.data_ptr(), am_out.data_ptr(),
             lm_out.data_ptr(), total.data_ptr(), order.data_ptr(), n_scored.data_ptr(), _stream())
    return lm, (ids_out, len_out, am_out, lm_out, total, order, n_scored)


# ---- edit distance, MBR ranking and the MWER terms (csrc/editdist.hip; semantics: include/franken_hip.h) ----

def edit_distance_route(La: int, Lb: int) -> int:
    """The kernel a pair of row widths takes (fk_edit_distance_route; host-side query, no launch): EDIT_LANE with min(La, Lb) <= 64,
    EDIT_ROWS4 up to 256, EDIT_ROWS16 up to 1024; raises outside 1 .. NBEST_MAX_T."""
    rc = lib().fk_edit_distance_route(La, Lb)
    _lib.check(0 if rc >= 0 else rc, "fk_edit_distance_route")
    return rc


def _edit_seqs(t: Tensor, lens: Optional[Tensor], what: str):
    assert t.dim() == 3 and t.dtype == torch.int64 and t.stride(2) == 1, f"{what}: int64 [B, n, L] with unit token stride"
    if lens is not None:
        assert lens.dtype == torch.int64 and lens.shape == t.shape[:2] and lens.is_contiguous() and lens.device == t.device, \
            f"{what} lengths: contiguous int64 [B, n]"
    return t.shape


def _edit_ld(t: Tensor) -> Tuple[int, int]:
    """(batch stride, sequence stride) of int64 [B, n, L]; a dimension of one element may carry any stride, so it gets the dense one"""
    B, n, L = t.shape
    ldh = t.stride(1) if n > 1 else max(t.stride(1), L)
    return (t.stride(0) if B > 1 else max(t.stride(0), (n - 1) * ldh + L)), ldh


def edit_distance(a: Tensor, a_lengths: Optional[Tensor], b: Tensor, b_lengths: Optional[Tensor], pad_value: int = -100,
                  want_lengths: bool = False):
    """a int64 [B, n_a, La] (n_a = n or 1: the group's reference), b int64 [B, n, Lb], any batch and sequence stride; lengths int64 or None
    (a sequence ends at its first `pad_value`) -> dist int32 [B, n], and with want_lengths the measured lengths of a, int32 [B, n_a]
    (fk_edit_distance)."""
    B, n_a, La = _edit_seqs(a, a_lengths, "a")
    Bb, n, Lb = _edit_seqs(b, b_lengths, "b")
    assert B == Bb and a.device == b.device
    dist = torch.empty((B, n), dtype=torch.int32, device=b.device)
    alen_out = torch.empty((B, n_a), dtype=torch.int32, device=b.device) if want_lengths else None
    with _timed("edit_distance"):
        call("fk_edit_distance", a.data_ptr(), *_edit_ld(a), _ptr(a_lengths), n_a, La, b.data_ptr(), *_edit_ld(b), _ptr(b_lengths), Lb, B, n,
             pad_value, dist.data_ptr(), _ptr(alen_out), _stream())
    return (dist, alen_out) if want_lengths else dist


def nbest_pairwise_distance(ids: Tensor, lengths: Tensor, scores: Optional[Tensor]) -> Tensor:
    """All pairwise distances inside every sentence's list -> int32 [B, n, n], -1 in the row and column of a hypothesis whose score is not
    finite (fk_nbest_pairwise_distance)."""
    B, n, T = _nbest_ids(ids, lengths, scores)
    dist = torch.empty((B, n, n), dtype=torch.int32, device=ids.device)
    with _timed("nbest_pairwise_distance"):
        call("fk_nbest_pairwise_distance", ids.data_ptr(), *_edit_ld(ids), lengths.data_ptr(), _ptr(scores), B, n, T, dist.data_ptr(), _stream())
    return dist


def mbr_rank(dist: Tensor, ids: Tensor, lengths: Tensor, scores: Tensor, scale: float = 1.0, pad: int = -100):
    """dist int32 [B, n, n] of nbest_pairwise_distance -> (risk fp32 [B, n] in input order, ranked) with ranked = (ids [B, n, T] padded with
    `pad`, lengths, scores, risk, order int64 [B, n], n_valid int64 [B]) in the order of ascending expected distance (fk_mbr_rank)."""
    B, n, T = _nbest_ids(ids, lengths, scores)
    assert scores is not None and dist.dtype == torch.int32 and dist.shape == (B, n, n) and dist.is_contiguous()
    dev = ids.device
    risk, sc_out, risk_out = (torch.empty((B, n), dtype=torch.float32, device=dev) for _ in range(3))
    ids_out = torch.empty((B, n, T), dtype=torch.int64, device=dev)
    len_out, order = (torch.empty((B, n), dtype=torch.int64, device=dev) for _ in range(2))
    n_valid = torch.empty(B, dtype=torch.int64, device=dev)
    with _timed("mbr_rank"):
        call("fk_mbr_rank", dist.data_ptr(), scores.data_ptr(), float(scale), ids.data_ptr(), *_edit_ld(ids), lengths.data_ptr(), B, n, T,
             pad, risk.data_ptr(), ids_out.data_ptr(), len_out.data_ptr(), sc_out.data_ptr(), risk_out.data_ptr(), order.data_ptr(),
             n_valid.data_ptr(), _stream())
    return risk, (ids_out, len_out, sc_out, risk_out, order, n_valid)


def mwer_combine(nll: Tensor, errors: Tensor, scores: Optional[Tensor] = None, lengths: Optional[Tensor] = None, max_len: int = 255):
    """nll fp32 [B, n], errors int32 [B, n], scores fp32 [B, n] / lengths int64 [B, n] or None -> (loss fp32 [B], coef fp32 [B, n] = d loss /
    d nll, count fp32 [1] = the sentences with a valid hypothesis, valid uint8 [B, n]) (fk_mwer_combine)."""
    assert nll.dim() == 2 and nll.dtype == torch.float32 and nll.is_contiguous()
    B, n = nll.shape
    assert errors.dtype == torch.int32 and errors.shape == (B, n) and errors.is_contiguous()
    assert scores is None or (scores.dtype == torch.float32 and scores.shape == (B, n) and scores.is_contiguous())
    assert lengths is None or (lengths.dtype == torch.int64 and lengths.shape == (B, n) and lengths.is_contiguous())
    dev = nll.device
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    coef = torch.empty((B, n), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.float32, device=dev)
    valid = torch.empty((B, n), dtype=torch.uint8, device=dev)
    with _timed("mwer_combine"):
        call("fk_mwer_combine", nll.data_ptr(), errors.data_ptr(), _ptr(scores), _ptr(lengths), max_len, B, n, loss.data_ptr(), coef.data_ptr(),
             count.data_ptr(), valid.data_ptr(), _stream())
    return loss, coef, count, valid


def mwer_reduce_rows(rows: Tensor, valid: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """rows [B * n, ...] (fp32 / bf16, contiguous: the gradient of logits expanded n times), valid uint8 [B, n] -> out [B, ...]: the valid
    rows of every sentence added in a fixed order, on top of `out` with accumulate (fk_mwer_reduce_rows).  An invalid row is never read."""
    B, n = valid.shape
    assert valid.dtype == torch.uint8 and valid.is_contiguous() and rows.is_contiguous() and rows.shape[0] == B * n
    if out is None:
        assert not accumulate
        out = torch.empty((B, *rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    assert out.is_contiguous() and out.dtype == rows.dtype and out.numel() * n == rows.numel()
    with _timed("mwer_reduce_rows"):
        call("fk_mwer_reduce_rows", rows.data_ptr(), valid.data_ptr(), out.data_ptr(), B, n, rows.numel() // (B * n), int(accumulate), fk_dtype(rows),
             _stream())
    return out
