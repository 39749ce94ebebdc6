"""Greedy decoding rate of the GPT decoder through the public `generate` API only (so the same file runs on any commit):

    python tools/decode_bench.py --model gpt2 --batch 1        # GPT-2 124M, the reference's decoder (franky_baseline_gpt2.ipynb)
    python tools/decode_bench.py --model nano --all-modes       # cfg1's gpt2-nano: re-forward vs kv-cache vs kv-cache + hipGraph
    python tools/decode_bench.py --model gpt2 --beam 5 --topk 20 --new-tokens 25     # generate_beam_search: cached (+ hipGraph) vs re-forward
    python tools/decode_bench.py --model gpt2 --beam 5 --sentences 1,2,3,4,8,16 --new-tokens 25    # S sentences in one search vs S searches

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


def beam_bench(g, a, prefix, start):
    """generate_beam_search of width --beam: cached + hipGraph, cached eager and the re-forward loop (use_cache=False) in one process, the
    repeats of the modes interleaved so that a drift of the machine hits all of them; beside them generate() at batch = beam width in
    graph mode, the same decode step without the two beam launches.  Per-step figures are marginal like the per-token ones: (time of N
    new tokens - time of N/4) / (3N/4); for the re-forward loop, whose steps grow with the sequence, that is the mean step between
    N/4 and N."""
    W, n, n4 = a.beam, a.new_tokens, max(1, a.new_tokens // 4)
    beam = lambda kw: (lambda k: g.generate_beam_search(start, k, prefix, topk=a.topk, beam_width=W, **kw))
    startW, prefixW = start.repeat(W, 1), prefix.repeat(W, 1, 1)
    modes = {"beam kv-cache + hipGraph": beam(dict(use_cache=True, use_graph=True)),
             "beam kv-cache (eager)": beam(dict(use_cache=True, use_graph=False)),
             "beam re-forward": beam(dict(use_cache=False)),
             f"generate batch {W} + hipGraph": lambda k: g.generate(startW, k, prefix=prefixW, top_k=a.topk, use_cache=True, use_graph=True)}
    times = {name: {n4: [], n: []} for name in modes}
    for name, fn in modes.items():                          # warm up both lengths of every mode
        for k in (n4, n):
            fn(k)
    for _ in range(a.repeats):
        for k in (n4, n):
            for name, fn in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(k)
                torch.cuda.synchronize()
                times[name][k].append(time.perf_counter() - t0)
    steps = {}
    for name in modes:
        t4, t = statistics.median(times[name][n4]), statistics.median(times[name][n])
        steps[name] = (t - t4) / (n - n4) if n > n4 else t / n
        print(f"{name:30s}: {steps[name] * 1e6:9.1f} us/step (marginal)   | whole call {t * 1e3:8.2f} ms [{min(times[name][n]) * 1e3:.2f} .. "
              f"{max(times[name][n]) * 1e3:.2f}], {n4} tokens {t4 * 1e3:8.2f} ms")
    ref = steps["beam re-forward"]
    print(f"re-forward / cached + hipGraph = {ref / steps['beam kv-cache + hipGraph']:.2f}x per step, re-forward / cached eager = "
          f"{ref / steps['beam kv-cache (eager)']:.2f}x; whole call {statistics.median(times['beam re-forward'][n]) / statistics.median(times['beam kv-cache + hipGraph'][n]):.2f}x "
          f"and {statistics.median(times['beam re-forward'][n]) / statistics.median(times['beam kv-cache (eager)'][n]):.2f}x")


def sentences_bench(g, a, d_model):
    """--beam W --sentences S[,S..]: the cached beam search of S sentences in ONE call (S * W rows per step) beside S sequential
    one-sentence calls, each as a hipGraph and eager, in one process with the repeats of the four modes interleaved.  sentences/s is the
    whole call (prefill and capture included); us/step is marginal, (time of N new tokens - time of N/4) / (3N/4), and for the sequential
    loop it is the step of ONE of its sentences, S of which make a step of the loop."""
    W, n, n4 = a.beam, a.new_tokens, max(1, a.new_tokens // 4)
    print(f"{'S':>3s} {'rows':>4s}  {'mode':32s} {'us/step':>9s} {'call ms':>9s} {'[min .. max]':>19s} {'sentences/s':>11s}")
    for S in a.sentences:
        prefix = torch.randn(S, 32, d_model, device="cuda")
        start = torch.full((S, 1), 50256, dtype=torch.long, device="cuda")

        def batched(kw):
            return lambda k: g.generate_beam_search(start, k, prefix, topk=a.topk, beam_width=W, use_cache=True, **kw)

        def sequential(kw):
            def run(k):
                for i in range(S):
                    g.generate_beam_search(start[i:i + 1], k, prefix[i:i + 1], topk=a.topk, beam_width=W, use_cache=True, **kw)
            return run

        modes = {"batched + hipGraph": batched(dict(use_graph=True)), "batched eager": batched(dict(use_graph=False)),
                 "sequential + hipGraph": sequential(dict(use_graph=True)), "sequential eager": sequential(dict(use_graph=False))}
        times = {name: {n4: [], n: []} for name in modes}
        for name, fn in modes.items():                      # warm up both lengths of every mode
            for k in (n4, n):
                fn(k)
        for _ in range(a.repeats):
            for k in (n4, n):
                for name, fn in modes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(k)
                    torch.cuda.synchronize()
                    times[name][k].append(time.perf_counter() - t0)
        for name in modes:
            t4, t = statistics.median(times[name][n4]), statistics.median(times[name][n])
            step = ((t - t4) / (n - n4) if n > n4 else t / n) / (S if name.startswith("sequential") else 1)
            print(f"{S:3d} {S * W:4d}  {name:32s} {step * 1e6:9.1f} {t * 1e3:9.2f} {f'[{min(times[name][n]) * 1e3:.2f} .. {max(times[name][n]) * 1e3:.2f}]':>19s} "
                  f"{S / t:11.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=sorted(MODELS), default="nano")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--new-tokens", type=int, default=200)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--all-modes", action="store_true", help="also time the full re-forward and the eager kv-cache loop (default: hipGraph only)")
    ap.add_argument("--beam", type=int, default=0, help="beam width: time generate_beam_search (cached + hipGraph, cached eager, re-forward) instead of generate")
    ap.add_argument("--topk", type=int, default=20, help="top-k of the beam search's draws (with --beam)")
    ap.add_argument("--sentences", type=lambda v: [int(x) for x in v.split(",")], default=None,
                    help="with --beam: sentences per batched search, one or a comma-separated list; each beside as many one-sentence searches")
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
    if a.beam and a.sentences:
        print(f"beam width {a.beam}, topk {a.topk}, sentences {a.sentences}")
        return sentences_bench(g, a, m["n_embd"])
    if a.beam:
        if B != 1:
            ap.error("--beam with --batch: give the number of sentences as --sentences")
        print(f"beam width {a.beam}, topk {a.topk}")
        return beam_bench(g, a, prefix, start)
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
