"""Shared parity cases: the configs the golden fixtures were generated with
(tests/golden/make_golden.py) expressed for the oracle, plus seeded inputs."""
from __future__ import annotations

import numpy as np
import torch

from frankenstein_amd import synth
from oracle import ref_models as R


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def state(shapes, seed=synth.SEED_WEIGHTS):
    return {k: t(v) for k, v in synth.make_state(shapes, seed).items()}


def enc_small():
    return R.mae_config(window_size=32, n_electrodes=16, patch_size=4, dim=64, n_layers=2, head_dim=16,
                        hidden_dim=128, n_heads=4, n_kv_heads=4)


def bf_l1_small():
    cfg = R.perceiver_config(enc_small(), n_output_tokens=8, output_dim=12, dim=64, n_layers=2, head_dim=8,
                             hidden_dim=96, n_heads=4, n_kv_heads=4)
    x = t(synth.make_inputs(3, 32, 16))
    tgt = t(synth.make_motion_targets(3, 8, 12))
    return cfg, x, tgt


def bf_ce_small():
    cfg = R.perceiver_config(enc_small(), n_output_tokens=7, output_dim=300, dim=64, n_layers=1, head_dim=16,
                             hidden_dim=96, n_heads=4, n_kv_heads=4)
    x = t(synth.make_inputs(3, 32, 16))
    tok = t(synth.make_tokens(3, 7, vocab=300))
    return cfg, x, tok


def gpt_small(bias: bool):
    cfg = R.gpt_config(block_size=64, vocab_size=211, n_layer=2, n_head=4, n_embd=64, dropout=0.0, bias=bias)
    prefix = t(synth.make_motion_targets(3, 5, 64, seed=99))
    tk = t(synth.make_tokens(3, 9, vocab=211))
    idx = tk.clone()
    idx[idx == -100] = 210
    return cfg, prefix, tk, idx


def cfg1():
    enc = R.mae_config(window_size=200, n_electrodes=256, patch_size=25, dim=128, n_layers=2, head_dim=32,
                       hidden_dim=512, n_heads=4, n_kv_heads=4)
    bcfg = R.perceiver_config(enc, n_output_tokens=32, output_dim=128, dim=128, n_layers=2, head_dim=32,
                              hidden_dim=256, n_heads=4, n_kv_heads=4)
    gcfg = R.gpt_config(block_size=1024, vocab_size=50257, n_layer=2, n_head=4, n_embd=128, dropout=0.0, bias=True)
    x = t(synth.make_inputs(4, 200, 256))
    tok = t(synth.make_tokens(4, 25))
    return bcfg, gcfg, x, tok


def cfg1_shapes(bcfg, gcfg):
    s = R.brainformer_shapes(bcfg, "to_words", p="brain_model.")
    s.update(R.gpt_shapes(gcfg, p="llm_model."))
    return s


def cfg2(B=1, head_dim_out=128):
    enc = R.mae_config(window_size=600, n_electrodes=256, patch_size=25, dim=384, n_layers=6, head_dim=64,
                       hidden_dim=1536, n_heads=6, n_kv_heads=6)
    cfg = R.perceiver_config(enc, n_output_tokens=32, output_dim=head_dim_out, dim=384, n_layers=2, head_dim=64,
                             hidden_dim=768, n_heads=6, n_kv_heads=6)
    x = t(synth.make_inputs(B, 600, 256))
    tgt = t(synth.make_motion_targets(B, 32, head_dim_out))
    return cfg, x, tgt


def summarize_rows(named):
    names, rows = [], []
    for k, v in named.items():
        a = v.detach().double().flatten().numpy()
        head = np.zeros(8)
        head[: min(8, a.size)] = a[:8]
        names.append(k)
        rows.append(np.concatenate([[a.sum(), np.abs(a).sum()], head]))
    return names, np.array(rows)


def sample_index(n: int, k: int = 256) -> np.ndarray:
    """k evenly spaced flat indices of an n-element tensor (all of them when n <= k): the gradient samples stored for the
    full-size fixtures, whose complete gradients would be tens of MB."""
    return np.arange(n) if n <= k else (np.arange(k, dtype=np.int64) * n) // k


def sample_rows(named, k: int = 256):
    """name -> float64 [k] sample of the flattened tensor (zero padded below k elements)."""
    names, rows = [], []
    for key, v in named.items():
        a = v.detach().double().flatten().numpy()
        r = np.zeros(k)
        idx = sample_index(a.size, k)
        r[: idx.size] = a[idx]
        names.append(key)
        rows.append(r)
    return names, np.array(rows)


def cfg2_ce(B=1):
    """cfg2's CE-head variant (notebook class, n_output_tokens=25, output_dim=50257)."""
    enc = R.mae_config(window_size=600, n_electrodes=256, patch_size=25, dim=384, n_layers=6, head_dim=64,
                       hidden_dim=1536, n_heads=6, n_kv_heads=6)
    cfg = R.perceiver_config(enc, n_output_tokens=25, output_dim=50257, dim=384, n_layers=2, head_dim=64,
                             hidden_dim=768, n_heads=6, n_kv_heads=6)
    x = t(synth.make_inputs(B, 600, 256))
    tok = t(synth.make_tokens(B, 25))
    return cfg, x, tok


def mae_small():
    cfg = R.mae_config(window_size=32, n_electrodes=16, patch_size=4, dim=64, n_layers=2, head_dim=16, hidden_dim=128,
                       n_heads=4, n_kv_heads=4, n_dec_layers=2, decoder_dim=64)
    return cfg, t(synth.make_inputs(3, 32, 16))


def unpatch(tok, C, P):
    """'b (t c) p -> b (t p) c' (models/brainformer.py:372)"""
    B, N, _ = tok.shape
    return tok.view(B, N // C, C, P).permute(0, 1, 3, 2).reshape(B, (N // C) * P, C)


def simple_mae_small():
    ecfg = R.simple_encoder_config(block_size=40, patch_size=24, n_layers=2, dim=64, hidden_dim=128, head_dim=16, n_heads=4, n_kv_heads=4)
    mcfg = R.simple_mae_config(n_layers=2, dim=48, hidden_dim=96, head_dim=8, n_heads=4, n_kv_heads=4)
    return ecfg, mcfg


def cfg5_simple_mae(pad_from=(600, 590, 333, 599)):
    """BASELINE configs[4] at SURVEY 8d's size (cfg5): SimpleMAE, 6-layer d = 384 encoder on 600 frame tokens, 2-layer decoder; the input
    of tests/golden/cfg5_simple_mae.npz: B = 4 synthetic samples, three of them with zero-padded tails."""
    ecfg = R.simple_encoder_config(block_size=600, patch_size=256, n_layers=6, dim=384, hidden_dim=1536, head_dim=64, n_heads=6, n_kv_heads=6)
    mcfg = R.simple_mae_config(n_layers=2, dim=384, hidden_dim=1536, head_dim=64, n_heads=6, n_kv_heads=6)
    x = t(synth.make_inputs(len(pad_from), 600, 256)).clone()
    for b, p0 in enumerate(pad_from):
        x[b, int(p0):] = 0.0
    return ecfg, mcfg, x


def train_accum(n_items: int = 10):
    """Dataset of the grad_accum fixture (tests/golden/train_accum.npz): sample i -> (x_i, y_i)."""
    cfg, _, _ = bf_l1_small()
    xs = t(synth.make_inputs(n_items, 32, 16, seed=synth.SEED_INPUT + 17))
    ys = t(synth.make_motion_targets(n_items, 8, 12, seed=synth.SEED_INPUT + 18))
    return cfg, xs, ys


# ------------------------------------------------------------------------------------------------ GEMM routes
# The shapes of tests/test_gemm_routes_gpu.py, shared with tests/test_gemm_routes_cpu.py, which pins the kernel each of them reaches
# (kernels.gemm_nt_route / gemm_tn_route).  Routes are named as in csrc/gemm.hip's NtRoute; "F32" = fp32 operands, the staged fp32 kernel.
# ring_min: the FK_NT_RING_MIN_TILES the case runs under ("0": every M >= 4096 shape is sent to the ring kernels; None: the default of 128
# tiles of 256 rows).  Rows are 4096 .. 8300 on the ring / NT_BIG routes and at most ~3100 elsewhere, every last row tile is ragged.

# plain / bias / residual / periodic residual: (route, M, N, K, ring_min)
NT_PLAIN_CASES = [
    ("NT_RING2", 4168, 256, 64, "0"),            # one k-stage
    ("NT_RING2", 8300, 1152, 384, None),         # default threshold (33 x 5 tiles), 6 stages, half-empty last column tile
    ("NT_RING192", 4168, 384, 64, "0"),
    ("NT_RING192", 4300, 576, 384, "0"),            # three 192-column tiles (N = 768 is NT_RING2's)
    ("NT_RING192", 4104, 192, 128, "0"),         # a single 192-column tile
    ("NT_RING128", 4168, 128, 64, "0"),
    ("NT_RING128", 4104, 640, 320, "0"),
    ("NT_RING128", 8300, 896, 192, None),        # default threshold (33 x 4 tiles of 256)
    ("NT_BIG", 4096 + 72, 256, 64, None),
    ("NT_BIG", 4096 + 72, 512, 384, None),
    ("NT_GLDS4", 300, 200, 64, None),
    ("NT_GLDS4", 1000, 1000, 128, None),
    ("NT_GLDS4", 700, 333, 192, None),           # N % 8 != 0: scalar sweep
    ("NT_GLDS", 2950, 1416, 64, None),           # 24 x 12 = 288 tiles (one per workgroup), N % 128 != 0, N % 8 == 0
    ("NT_GLDS", 2821, 3080, 128, None),          # 23 x 25 = 575 tiles on 512 workgroups: 1 or 2 tiles each, 8 does not divide the count
    ("NT_GLDS", 2950, 1413, 64, None),           # scalar sweep, clamped B rows in the last column tile
    ("NT_GLDS", 2821, 3077, 192, None),          # scalar sweep over the multi-tile loop
    ("NT_GLDS", 3100, 5760, 128, None),          # 25 x 45 = 1125 tiles: up to 3 per workgroup
    ("NT_STAGED", 300, 200, 8, None),
    ("NT_STAGED", 1000, 333, 72, None),
    ("NT_STAGED", 700, 520, 200, None),
    ("F32", 300, 200, 4, None),
    ("F32", 700, 333, 36, None),
    ("F32", 1000, 520, 100, None),
]

# SwiGLU forward (N = 2H columns): (route, M, H, K, ring_min)
NT_SWIGLU_CASES = [
    ("NT_RING2", 4168, 128, 128, "0"),
    ("NT_RING2", 4200, 576, 64, "0"),            # N = 1152
    ("NT_RING128", 4168, 192, 64, "0"),          # N = 384: the fused modes are kept off the 192-column tiles
    ("NT_BIG", 4168, 128, 64, None),
    ("NT_GLDS", 2950, 712, 64, None),            # N = 1424: 24 x 12 = 288 tiles
    ("NT_GLDS4", 300, 96, 64, None),
    ("NT_STAGED", 300, 96, 72, None),
    ("F32", 300, 96, 36, None),
]

# SwiGLU backward (N = H accumulator columns, 2H columns of h13 / dh13): (route, M, H, K, ring_min)
NT_DSWIGLU_CASES = [
    ("NT_RING2", 4168, 256, 64, "0"),
    ("NT_RING128", 4168, 384, 128, "0"),
    ("NT_RING128", 4200, 128, 384, "0"),
    ("NT_BIG", 4168, 256, 128, None),
    ("NT_GLDS", 2950, 1416, 64, None),
    ("NT_GLDS4", 300, 96, 64, None),
    ("NT_STAGED", 300, 96, 72, None),
    ("F32", 300, 96, 36, None),
]

# RoPE: (route, B, T, N, K, D, rot_cols, pos_off, q_cols, bias, per_sample_table, ring_min); M = B * T.  T = 5 (the table wrap runs more
# than once per 8-row step), 57 (not a multiple of 8) and 300 (more than a row tile); q_cols > 0: those columns use the pre-scaled table
NT_ROPE_CASES = [
    ("NT_RING2", 821, 5, 256, 64, 8, 256, 3, 0, True, True, "0"),
    ("NT_RING2", 14, 300, 512, 128, 128, 256, 0, 128, False, False, "0"),
    ("NT_RING2", 73, 57, 1152, 64, 64, 768, 7, 384, False, True, "0"),
    ("NT_RING128", 73, 57, 384, 64, 64, 256, 2, 128, True, True, "0"),
    ("NT_RING128", 821, 5, 128, 384, 16, 128, 0, 0, False, False, "0"),
    ("NT_RING128", 14, 300, 384, 128, 8, 384, 11, 0, False, True, "0"),
    ("NT_BIG", 73, 57, 256, 64, 16, 192, 5, 64, True, True, None),
    ("NT_BIG", 14, 300, 512, 64, 64, 512, 0, 0, False, False, None),
    ("NT_BIG", 821, 5, 256, 128, 128, 128, 1, 0, False, True, None),
    ("NT_GLDS", 10, 300, 1416, 64, 8, 1408, 4, 0, True, True, None),
    ("NT_GLDS", 590, 5, 1416, 64, 64, 1408, 0, 704, False, False, None),
    ("NT_GLDS", 50, 57, 1416, 128, 16, 1416 - 8, 9, 0, False, True, None),
    ("NT_GLDS4", 4, 57, 200, 64, 8, 200, 6, 0, False, True, None),
    ("NT_GLDS4", 60, 5, 384, 128, 128, 256, 2, 128, True, True, None),
    ("NT_GLDS4", 3, 300, 192, 64, 64, 128, 0, 0, False, False, None),
    ("NT_STAGED", 4, 57, 192, 72, 16, 128, 3, 64, True, True, None),
    ("NT_STAGED", 60, 5, 256, 200, 128, 256, 0, 0, False, False, None),
    ("F32", 60, 5, 192, 36, 64, 192, 1, 64, True, True, None),
    ("F32", 2, 300, 128, 100, 8, 96, 0, 0, False, False, None),
    ("F32", 4, 57, 256, 36, 128, 256, 4, 0, False, True, None),
]

# fk_gemm_tn: (kernel, dtype, M, N1, N2, nsplit, rows_per_split); kernel 0 = the 128 x 128 kernel, 128 / 192 = the large-tile kernel
TN_CASES = [
    (0, "bf16", 200, 136, 72, 1, 256),           # nsplit == 1: the kernel writes / accumulates into C itself
    (0, "f32", 100, 136, 72, 1, 128),
    (0, "bf16", 1000, 136, 72, 4, 256),
    (0, "f32", 1000, 136, 72, 8, 128),
    (0, "bf16", 4163, 904, 1000, 16, 320),       # splits 0 .. 12 full, split 13 has 3 rows, splits 14 and 15 start past M
    (0, "f32", 2083, 904, 1000, 16, 160),        # the same in fp32: split 13 has 3 rows, 14 and 15 are empty
    (128, "bf16", 16384, 384, 128, 32, 512),
]


# ------------------------------------------------------------------------------------------------ attention routes
# The shapes of tests/test_attn_routes_gpu.py, shared with tests/test_attn_routes_cpu.py, which pins the (forward, dQ, dK/dV) kernels each
# of them reaches (kernels.attn_route) and checks that the inputs of tests/attn_inputs.py turn a lost key into a gross error on it.
# mask: ("none",) | ("causal",) | ("block", c) | ("sliced", "causal" | "block", c, full_q, full_k) (the [-Nq:, -Nk:] slice of a full mask:
# position offsets) | ("prefix", block, n_full) (MAE sub-mask of sorted token ids) | ("keypad",) | ("dense", Bm, Hm) (1 = broadcast).
# ps: FK_ATTN_Q_PRESCALED (bf16, D = 64).
def _attn(dtype, B, H, Nq, Nk, D, mask, routes, ps=False, **kw):
    name = "-".join([".".join(routes), dtype, f"{B}x{H}x{Nq}x{Nk}x{D}", "_".join(map(str, mask))]
                    + (["ps"] if ps else []) + [f"{k}{v}" for k, v in kw.items()])
    return dict(id=name, dtype=dtype, B=B, H=H, Nq=Nq, Nk=Nk, D=D, mask=mask, routes=routes, ps=ps, **kw)


_GEN = ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC")
_FEWQ = ("FWD_FEWQ", "DQ_FEWQ", "DKDV_GENERIC")
_PS = ("FWD_PS", "DQ_PS", "DKDV_PS")
ATTN_ROUTE_CASES = [
    # generic kernels: fp32 D 8 / 16 / 32 / 64, bf16 D 8 / 16 / 32 / 64 / 128, every mask kind, ragged, more than one workgroup
    _attn("f32", 2, 3, 40, 130, 8, ("none",), _GEN),
    _attn("f32", 2, 2, 150, 150, 16, ("causal",), _GEN),
    _attn("f32", 1, 2, 40, 200, 32, ("sliced", "block", 8, 256, 256), _GEN),
    _attn("f32", 2, 2, 70, 100, 64, ("dense", 2, 2), _GEN),
    _attn("f32", 2, 2, 139, 139, 32, ("keypad",), _GEN),
    _attn("bf16", 2, 2, 130, 130, 8, ("keypad",), _GEN),
    _attn("bf16", 2, 2, 140, 140, 16, ("prefix", 16, 400), _GEN),
    _attn("bf16", 2, 3, 70, 100, 32, ("dense", 1, 3), _GEN),
    _attn("bf16", 2, 2, 200, 200, 128, ("causal",), _GEN),
    _attn("bf16", 2, 2, 130, 130, 64, ("block", 16), _GEN),
    _attn("bf16", 1, 2, 150, 90, 64, ("dense", 1, 1), _GEN),
    # few queries, long context: the waves split the keys (forward and dQ)
    _attn("bf16", 2, 2, 8, 1024, 64, ("none",), _FEWQ),
    _attn("bf16", 2, 2, 32, 1100, 64, ("none",), _FEWQ),
    # the pre-scaled tile loops: ragged, causal, block-causal 8 and 128, sliced offsets, prefix and key-padding tables
    _attn("bf16", 2, 2, 333, 333, 64, ("causal",), _PS, ps=True),
    _attn("bf16", 2, 2, 200, 200, 64, ("block", 8), _PS, ps=True),
    _attn("bf16", 1, 2, 300, 300, 64, ("block", 128), _PS, ps=True),
    _attn("bf16", 1, 2, 40, 300, 64, ("none",), _PS, ps=True),
    _attn("bf16", 2, 2, 256, 384, 64, ("sliced", "block", 128, 512, 512), _PS, ps=True),
    _attn("bf16", 2, 2, 260, 260, 64, ("prefix", 16, 700), _PS, ps=True),
    _attn("bf16", 2, 2, 270, 270, 64, ("keypad",), _PS, ps=True),
    _attn("bf16", 2, 1, 1100, 1100, 64, ("keypad",), _PS, ps=True),
    # the generated forward and dQ streams (128 queries per workgroup, 64-key tiles): 1 .. 9 key tiles, every ring phase; dK/dV takes the
    # narrow stream at Nk % 128 == 0 (2 query tiles), the wide one at Nk % 256 == 0, the tile loop otherwise
    _attn("bf16", 2, 2, 128, 64, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_PS"), ps=True),
    _attn("bf16", 2, 2, 128, 128, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_ASM"), ps=True),
    _attn("bf16", 1, 2, 128, 192, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_PS"), ps=True),
    _attn("bf16", 2, 2, 128, 256, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDVW_ASM"), ps=True),
    _attn("bf16", 2, 1, 128, 320, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_PS"), ps=True),
    _attn("bf16", 1, 2, 128, 384, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_ASM"), ps=True),
    _attn("bf16", 1, 1, 128, 448, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_PS"), ps=True),
    _attn("bf16", 1, 2, 256, 512, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDVW_ASM"), ps=True),
    _attn("bf16", 1, 2, 128, 576, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_PS"), ps=True),
    # the narrow dK/dV stream (64 queries per tile): 1 and 5 query tiles (2 above), and block-causal 128: 6, 4, 2 tiles
    _attn("bf16", 2, 2, 64, 128, 64, ("none",), ("FWD_PS", "DQ_PS", "DKDV_ASM"), ps=True),
    _attn("bf16", 1, 3, 320, 128, 64, ("none",), ("FWD_PS", "DQ_PS", "DKDV_ASM"), ps=True),
    _attn("bf16", 2, 2, 384, 384, 64, ("block", 128), ("FWD_ASM", "DQ_ASM", "DKDV_ASM"), ps=True),
    # the wide dK/dV stream (ring of 3 query tiles): 1, 3, 4, 7 query tiles (2 above), and block-causal 256: 8 and 4 tiles
    _attn("bf16", 2, 2, 64, 256, 64, ("none",), ("FWD_PS", "DQ_PS", "DKDVW_ASM"), ps=True),
    _attn("bf16", 2, 1, 192, 256, 64, ("none",), ("FWD_PS", "DQ_PS", "DKDVW_ASM"), ps=True),
    _attn("bf16", 1, 2, 256, 256, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDVW_ASM"), ps=True),
    _attn("bf16", 1, 2, 448, 256, 64, ("none",), ("FWD_PS", "DQ_PS", "DKDVW_ASM"), ps=True),
    _attn("bf16", 2, 2, 512, 512, 64, ("block", 256), ("FWD_ASM", "DQ_ASM", "DKDVW_ASM"), ps=True),
]

# online-softmax stress on the pre-scaled forward kernels (GPU file; the CPU file pins their routes): spike > 0: one late key outscores
# everything its row has seen by far (reference-0 loop -> exact loop, and on the generated stream the workgroup's redo); spike < 0: every
# score of head 0 lies that many log2 units down, far below the window of reference 0 (the classic loop throughout)
ATTN_SPIKE_CASES = [
    _attn("bf16", 1, 2, 200, 330, 64, ("none",), _PS, ps=True, spike=40.0),
    _attn("bf16", 1, 2, 384, 384, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDV_ASM"), ps=True, spike=40.0),
    _attn("bf16", 1, 2, 200, 200, 64, ("block", 8), _PS, ps=True, spike=-2048.0),
    _attn("bf16", 1, 2, 256, 256, 64, ("none",), ("FWD_ASM", "DQ_ASM", "DKDVW_ASM"), ps=True, spike=-2048.0),
]

# attn_bwd with a rope_table: the inverse rotation fused into the dQ / dK stores (tests/test_attn_rope_gpu.py; tests/test_attn_rope_cpu.py
# pins the routes, what the list covers, and that a wrong rotation is a gross error on every case).  Self-attention (Nq = Nk = N), q | k | v
# and dq | dk | dv views of one buffer each, as engine.AttnBranch.run_backward calls it.  routes: kernels.attn_route_names(..., rope=True).
# table: "shared" [Tc, D/2, 2] | "sample" [B, Tc, D/2, 2] | "strided" (the [:, :Tc] slice of a taller per-sample buffer: batch stride
# > Tc * D); Tc = rope_off + N (Rope.pos_off); seed: of the table's angles (attn_inputs.rope_table)
def _rope(dtype, B, H, N, D, mask, routes, table, rope_off, ps=False, seed=0):
    c = _attn(dtype, B, H, N, N, D, mask, routes, ps=ps)
    c.update(id=f"{c['id']}-{table}-off{rope_off}", table=table, rope_off=rope_off, seed=1000 + seed)
    return c


_ASM = ("FWD_ASM", "DQ_ASM")
ATTN_ROPE_CASES = [
    # bf16 D = 64, pre-scaled queries: the generated streams (narrow and wide dK/dV, full and block-causal) ..
    _rope("bf16", 2, 2, 128, 64, ("none",), _ASM + ("DKDV_ASM",), "shared", 0, ps=True),
    _rope("bf16", 2, 2, 256, 64, ("none",), _ASM + ("DKDVW_ASM",), "strided", 0, ps=True),
    _rope("bf16", 2, 2, 384, 64, ("block", 128), _ASM + ("DKDV_ASM",), "sample", 5, ps=True),
    _rope("bf16", 2, 2, 512, 64, ("block", 256), _ASM + ("DKDVW_ASM",), "shared", 3, ps=True),
    # .. and the tile loops: whole tiles, ragged, every analytic and table mask, position offsets in the mask and in the table at once
    _rope("bf16", 2, 3, 192, 64, ("none",), _PS, "shared", 0, ps=True),
    _rope("bf16", 2, 2, 200, 64, ("block", 8), _PS, "sample", 7, ps=True),
    _rope("bf16", 2, 2, 333, 64, ("causal",), _PS, "strided", 0, ps=True),
    _rope("bf16", 2, 2, 256, 64, ("sliced", "block", 128, 512, 512), _PS, "shared", 256, ps=True),
    _rope("bf16", 2, 2, 260, 64, ("prefix", 16, 700), _PS, "sample", 1, ps=True),
    _rope("bf16", 2, 2, 270, 64, ("keypad",), _PS, "shared", 9, ps=True),
    # bf16 D = 64, queries not pre-scaled, dense mask: the generic kernels on the swizzled image (the engine's "rope" path)
    _rope("bf16", 2, 2, 100, 64, ("dense", 2, 2), _GEN, "sample", 3),
    # the generic kernels: fp32 D 8 / 16 / 32 / 64, bf16 D 8 (scalar bf16x4 store) / 16 / 32 / 128, ragged N, more than one workgroup
    _rope("f32", 2, 3, 70, 8, ("causal",), _GEN, "sample", 3),
    _rope("f32", 2, 2, 150, 16, ("keypad",), _GEN, "shared", 0),
    _rope("f32", 2, 2, 90, 32, ("prefix", 16, 300), _GEN, "strided", 0),
    _rope("f32", 1, 2, 133, 64, ("block", 16), _GEN, "shared", 5),
    _rope("bf16", 2, 2, 130, 8, ("keypad",), _GEN, "sample", 1),
    _rope("bf16", 2, 2, 140, 16, ("prefix", 16, 400), _GEN, "shared", 0),
    _rope("bf16", 2, 3, 75, 32, ("causal",), _GEN, "strided", 0),
    _rope("bf16", 2, 2, 200, 128, ("block", 8), _GEN, "shared", 7),
]

# attn_fwd / attn_bwd with a dropout tuple (tests/test_attn_drop_gpu.py; tests/test_attn_drop_cpu.py pins the routes, what the list covers,
# and that a keep mask wrong in any way, down to one bit, is a gross error on every case).  Dropout runs on the generic kernels only
# (kernels.attn_route_names(..., dropout=True)).  p: drop probability; seed, step: the two seed words on the device; site: the number of
# the application within the forward (step and site nonzero; a RoPE case draws its table's angles from the same seed).  layout: "split" =
# q in its own buffer, k | v side by side, as in the route tests; "qkv" = q | k | v and dq | dk | dv views of one [B, N, 3 H D] buffer each,
# as engine.AttnBranch passes them (Nq = Nk).  table / rope_off as in _rope: attn_bwd gets the table together with the dropout tuple.
def _drop(dtype, B, H, Nq, Nk, D, mask, p, layout="split", seed=424242, step=9, site=2, table=None, rope_off=0):
    c = _attn(dtype, B, H, Nq, Nk, D, mask, _GEN)
    c.update(id=f"{dtype}-{B}x{H}x{Nq}x{Nk}x{D}-{'_'.join(map(str, mask))}-p{p}-{layout}-{seed}.{step}.{site}"
                + (f"-{table}-off{rope_off}" if table else ""), p=p, seed=seed, step=step, site=site, layout=layout)
    if table:
        c.update(table=table, rope_off=rope_off)
    return c


ATTN_DROP_ROWS = 1 << 16                 # the row-number case numbers its rows past this
ATTN_DROP_CASES = [
    # fp32 D 8 / 16 / 32 / 64, bf16 D 8 / 16 / 32 / 64 / 128; every mask kind, each at some p >= 0.25; ragged, Nq != Nk, p 0.1 .. 0.9
    _drop("f32", 2, 3, 40, 130, 8, ("none",), 0.5),
    _drop("f32", 2, 2, 150, 150, 16, ("causal",), 0.1, step=3, site=1),
    _drop("f32", 1, 2, 150, 200, 32, ("sliced", "causal", 0, 300, 260), 0.25),
    _drop("f32", 2, 2, 70, 100, 64, ("dense", 2, 2), 0.25, seed=77001, step=1, site=5),
    _drop("f32", 2, 2, 139, 139, 32, ("keypad",), 0.9),
    _drop("bf16", 2, 2, 130, 130, 8, ("keypad",), 0.25),
    _drop("bf16", 2, 2, 140, 140, 16, ("prefix", 16, 400), 0.5),
    _drop("bf16", 2, 3, 70, 100, 32, ("dense", 1, 3), 0.1),
    _drop("bf16", 2, 2, 200, 200, 128, ("causal",), 0.9, seed=5, step=70000, site=3),
    _drop("bf16", 2, 2, 130, 130, 64, ("block", 16), 0.5),
    _drop("bf16", 1, 2, 150, 90, 64, ("dense", 1, 1), 0.5),
    _drop("bf16", 2, 2, 150, 200, 32, ("sliced", "block", 8, 256, 256), 0.1),
    _drop("bf16", 2, 2, 150, 330, 16, ("none",), 0.25, site=7),
    # the engine's call: causal, D = 64, q | k | v and dq | dk | dv views of one buffer each, the product's p
    _drop("bf16", 2, 3, 300, 300, 64, ("causal",), 0.1, "qkv"),
    _drop("f32", 2, 2, 269, 269, 64, ("causal",), 0.1, "qkv"),
    # dropout together with the fused inverse RoPE of attn_bwd
    _drop("bf16", 2, 2, 200, 200, 64, ("block", 8), 0.25, "qkv", table="shared", rope_off=7),
    _drop("f32", 2, 2, 133, 133, 16, ("prefix", 16, 300), 0.5, "qkv", table="sample", rope_off=0),
    # row numbers (b H + h) Nq + q past 2^16: the only thing that tells the masks of two rows apart
    _drop("f32", 2, 3, 11100, 70, 8, ("none",), 0.5),
]
# the captured forward + backward of the GPU file's replay test: ~200 keys, the step word advanced on the device between the replays
ATTN_DROP_GRAPH_CASE = _drop("bf16", 2, 2, 200, 200, 64, ("causal",), 0.25, step=41, site=4)


# ------------------------------------------------------------------------------------------------ token-on-the-lane kernels
# The shapes of tests/test_lane_kernels_gpu.py (csrc/mlp_fused.hip: mlp_up_fused_kernel, qkv_rope_fused_kernel, mlp_bwd_fused_kernel and
# mlp_bwd_fused_asm_kernel), shared with tests/test_lane_routes_cpu.py, which pins the kernel each of them reaches
# (kernels.gemm_nt_swiglu_route / gemm_nt_rope_route / mlp_bwd_fused_route) and checks the inputs of tests/lane_ref.py against mutations
# of the float64 reference.  d = 384 everywhere.  The forward kernels take a call only when its 256-token workgroups fill at least 70 %
# of their rounds of 256 (mu_grid_fills): 45 825 .. 65 536 rows in one round, 91 649 .. 131 072 in two.
LANE_D = 384
LANE_M_ACCEPTED = ((45825, 65536), (91649, 131072))        # per number of rounds: first and last row count taken
LANE_M_REJECTED = ((1, 45824), (65537, 91648), (131073, 137472))

# up-projection + SwiGLU: (route, M, H).  H = 32 / 64 / 96 / 160: 1, 2, 3 and 5 chunks of 32 hidden units; M = 45 825 (one row in the
# last workgroup), 46 080 (whole workgroups), 49 007 (cuts an 8-row h13 store group and a 16-row g group); one two-round case
LANE_UP_CASES = [("NT_LANE", M, H) for H in (32, 64, 96, 160) for M in (45825, 46080, 49000 + 7)] + [("NT_LANE", 91649, 32)]

# q|k|v projection + RoPE, D = 64: (route, B, T, N, rot_cols, q_cols, pos_off, per_sample_table); the table has exactly pos_off + T rows
LANE_QKV_CASES = [
    ("NT_LANE", 45825, 1, 64, 0, 0, 0, False),
    ("NT_LANE", 47, 975, 64, 64, 0, 5, True),
    ("NT_LANE", 15275, 3, 64, 64, 64, 0, True),
    ("NT_LANE", 1, 45825, 64, 64, 64, 5, False),
    ("NT_LANE", 15275, 3, 192, 0, 0, 5, False),
    ("NT_LANE", 45825, 1, 192, 192, 0, 5, True),
    ("NT_LANE", 47, 975, 192, 192, 192, 0, False),
    ("NT_LANE", 1, 45825, 192, 128, 64, 0, True),
    ("NT_LANE", 47, 975, 384, 0, 0, 0, True),
    ("NT_LANE", 15275, 3, 384, 384, 0, 5, False),
    ("NT_LANE", 45825, 1, 384, 384, 384, 0, False),
    ("NT_LANE", 47, 975, 384, 256, 128, 5, True),
    ("NT_LANE", 15275, 3, 384, 256, 128, 0, True),
    ("NT_LANE", 1, 45825, 384, 256, 128, 5, False),
]

# the backward chain (fk_mlp_bwd_fused): (kernel, M, H); operands depend on H alone (the first M rows of 1024), so cases of one H are
# the same problem cut at different rows: (256, 64) on the generated stream and (255, 64) on the hipcc kernel are compared row for row
LANE_BWD_CASES = [
    ("MLP_BWD_HIPCC", 1, 32), ("MLP_BWD_HIPCC", 384 + 9, 32), ("MLP_BWD_ASM", 128, 32),
    ("MLP_BWD_HIPCC", 7, 64), ("MLP_BWD_HIPCC", 255, 64), ("MLP_BWD_ASM", 256, 64),
    ("MLP_BWD_HIPCC", 33, 96), ("MLP_BWD_HIPCC", 1000, 96), ("MLP_BWD_ASM", 128, 96),
    ("MLP_BWD_HIPCC", 127, 128), ("MLP_BWD_HIPCC", 384 + 9, 128), ("MLP_BWD_ASM", 256, 128),
    ("MLP_BWD_HIPCC", 129, 160), ("MLP_BWD_HIPCC", 7, 160), ("MLP_BWD_ASM", 256, 160),
]
LANE_BWD_ROWS = 1024                                        # rows the backward operands are drawn for
LANE_BWD_PAIR = (("MLP_BWD_ASM", 256, 64), ("MLP_BWD_HIPCC", 255, 64))

# saturated gates: pre-activations of exactly +-these values (both sides of __expf's overflow at 88.72)
LANE_SATURATED = (8, 16, 32, 64, 88, 96, 128)

# padded leading dimensions (test_padded_leading_dimensions): every operand and output of a call in a wider sentinel-filled buffer, pads
# of 8 .. 72 elements so that no two leading dimensions of a call are equal.  up: (M, H, pads of a, w13, h13, g); qkv: (B, T, N, rot, q,
# pos_off, per_sample, pads of a, w, out); backward: (M, H, pads of dy, w2t, h13, w13t, dh13, dx), a whole-tile and a ragged M
LANE_PAD_UP = (45825, 32, (8, 16, 24, 40))
LANE_PAD_QKV = (47, 975, 192, 128, 64, 5, True, (8, 16, 24))
LANE_PAD_BWD = [(128, 96, (8, 16, 24, 40, 56, 72)), (129, 96, (72, 56, 40, 24, 16, 8))]
