"""Greedy decoding rate of the GPT decoder through the public `generate` API only (so the same file runs on any commit):

    python tools/decode_bench.py --model gpt2 --batch 1        # GPT-2 124M, the reference's decoder (franky_baseline_gpt2.ipynb)
    python tools/decode_bench.py --model nano --all-modes       # cfg1's gpt2-nano: re-forward vs kv-cache vs kv-cache + hipGraph

Random weights, a 32-token brain prefix, one start token, top_k = 1.  A generate() call also pays the prefill and, in graph mode, the
capture, so the per-token figure is the MARGINAL cost: (time of N new tokens - time of N/4 new tokens) / (3N/4), medians over the
repeats, both lengths warmed up first.  The whole-call rate is printed beside it.

Ceiling: a decode step reads every weight matrix of the blocks and the (tied) head once, whatever the batch:
weight bytes / 6.29 TB/s (the MI355X copy peak); `fraction` = that time over the measured step time.  It is an end-to-end figure (the step
also runs attention over the cache, the embedding and the sampling), not a kernel's share of peak.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import frankenstein_amd as fa
from frankenstein_amd.models.gpt2_model import GPT, GPTConfig

HBM_PEAK = 6.29e12          # bytes/s, the measured copy peak of the MI355X
MODELS = {"nano": dict(n_layer=2, n_head=4, n_embd=128), "gpt2": dict(n_layer=12, n_head=12, n_embd=768)}
MODES = {"re-forward": dict(use_cache=False), "kv-cache": dict(use_cache=True, use_graph=False),
         "kv-cache + hipGraph": dict(use_cache=True, use_graph=True)}


def weight_bytes_per_step(g, esize):
    """bytes of the matrices a decode step streams: the four linears of every block and the vocabulary head (biases, norms: noise)"""
    n = sum(p.numel() for blk in g.transformer.h for p in (blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight))
    return (n + g.lm_head.weight.numel()) * esize


def timed(g, start, prefix, n_new, kw, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.generate(start, n_new, prefix=prefix, top_k=1, **kw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=sorted(MODELS), default="nano")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--new-tokens", type=int, default=200)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--all-modes", action="store_true", help="also time the full re-forward and the eager kv-cache loop (default: hipGraph only)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_bench needs the GPU"

    fa.set_compute_dtype(a.dtype)
    torch.manual_seed(0)
    m = MODELS[a.model]
    g = GPT(GPTConfig(block_size=1024, vocab_size=50257, dropout=0.0, bias=True, **m)).cuda().eval()
    B, n, n4 = a.batch, a.new_tokens, max(1, a.new_tokens // 4)
    prefix = torch.randn(B, 32, m["n_embd"], device="cuda")
    start = torch.full((B, 1), 50256, dtype=torch.long, device="cuda")
    wbytes = weight_bytes_per_step(g, 2 if a.dtype == "bf16" else 4)
    floor = wbytes / HBM_PEAK
    print(f"model {a.model} ({sum(p.numel() for p in g.parameters()) / 1e6:.1f} M parameters), {a.dtype}, batch {B}, {n} new tokens, "
          f"{a.repeats} repeats; weights per step {wbytes / 1e6:.1f} MB -> ceiling {floor * 1e6:.1f} us/step = {B / floor:.0f} tokens/s")
    for name, kw in MODES.items():
        if not a.all_modes and name != "kv-cache + hipGraph":
            continue
        for k in (n4, n):                                     # warm up both lengths (lazy weight shadows, allocator, code objects)
            g.generate(start, k, prefix=prefix, top_k=1, **kw)
        t4, _, _ = timed(g, start, prefix, n4, kw, a.repeats)
        t, lo, hi = timed(g, start, prefix, n, kw, a.repeats)
        step = (t - t4) / (n - n4) if n > n4 else t / n
        print(f"{name:20s}: {step * 1e6:9.1f} us/token (marginal)  {B / step:9.0f} tokens/s  fraction of the weight-streaming ceiling {floor / step:6.3f}"
              f"   | whole call {t * 1e3:8.1f} ms [{lo * 1e3:.1f} .. {hi * 1e3:.1f}] = {B * n / t:8.0f} tokens/s incl. prefill"
              + (" and capture" if kw.get("use_graph") else ""))


if __name__ == "__main__":
    main()
