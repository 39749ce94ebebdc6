"""Greedy decoding rate of the GPT decoder through the public `generate` API only (so the same file runs on any commit):

    python tools/decode_bench.py --model gpt2 --batch 1        # GPT-2 124M, the reference's decoder (franky_baseline_gpt2.ipynb)
    python tools/decode_bench.py --model nano --all-modes       # cfg1's gpt2-nano: re-forward vs kv-cache vs kv-cache + hipGraph
    python tools/decode_bench.py --model gpt2 --beam 5 --topk 20 --new-tokens 25     # generate_beam_search: cached (+ hipGraph) vs re-forward
    python tools/decode_bench.py --model gpt2 --beam 5 --sentences 1,2,3,4,8,16 --new-tokens 25    # S sentences in one search vs S searches
    python tools/decode_bench.py --model gpt2 --beam 5 --eos --new-tokens 25         # end-of-text: step, poll, early exit, device backtrack
    python tools/decode_bench.py --model gpt2 --batch 1 --top-p 0.9                  # nucleus sampling: the step with and without top_p
    python tools/decode_bench.py --model gpt2 --batch 1 --repetition-penalty 1.3 --no-repeat-ngram 3 --min-new-tokens 10    # the history rules
    python tools/decode_bench.py --model gpt2 --beam 5 --repetition-penalty 1.3 --no-repeat-ngram 3 --min-new-tokens 10     # ... in the beam search
    python tools/decode_bench.py --model gpt2 --beam 5 --ctc-weight 0.3 --sentences 1,3 --new-tokens 25    # joint CTC / attention decoding: the prefix scorer on and off

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


def eos_bench(g, a, prefix, start):
    """--beam W --eos: what the end-of-text path costs and saves, all as hipGraph searches in one process with the repeats interleaved.
    (1) the step with an end-of-text id that never ends anything against the plain step (marginal us/step), (2) the same search polled
    every 1, 8 and never (check_every), (3) a call in which every beam ends early (topk = W collapses the search to its greedy chain; the
    id is a token that chain first emits near the middle) against the plain call that runs all steps, (4) the host's walk through
    the logs of 3 sentences against fk_beam_backtrack."""
    from frankenstein_amd import kernels as K
    W, n, n4 = a.beam, a.new_tokens, max(1, a.new_tokens // 4)
    kw = dict(topk=a.topk, beam_width=W, use_cache=True, use_graph=True)
    never = 50255                                              # an id a random-weight decoder is unlikely to draw; last_steps shows whether it did
    ran = {}

    def eos_call(name, **extra):
        def fn(k):
            g.generate_beam_search(start, k, prefix, eos_token_id=never, **kw, **extra)
            ran[name] = g.last_steps
        return fn

    modes = {"plain": lambda k: g.generate_beam_search(start, k, prefix, **kw),
             "eos, check_every 1e9": eos_call("eos, check_every 1e9", check_every=10 ** 9),
             "eos, check_every 8": eos_call("eos, check_every 8", check_every=8),
             "eos, check_every 1": eos_call("eos, check_every 1", check_every=1)}
    times = {name: {n4: [], n: []} for name in modes}
    for fn in modes.values():
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
        print(f"{name:24s}: {(t - t4) / max(1, n - n4) * 1e6:9.1f} us/step (marginal) | whole call {t * 1e3:8.2f} ms [{min(times[name][n]) * 1e3:.2f} .. "
              f"{max(times[name][n]) * 1e3:.2f}]" + (f", ran {ran[name]} of {n} steps" if name in ran else ""), flush=True)
    # ---- (3) early exit: the greedy chain of the topk = W search and a token it first emits near the middle
    gk = dict(kw, topk=W)
    chain = g.generate_beam_search(start, n, prefix, **gk).cpu().tolist()[start.shape[1]:]
    js = [j for j in range(n // 3, n - 1) if chain[j] not in chain[:j]]
    if not js:
        print(f"early exit: the greedy chain of this model emits no new token between steps {n // 3} and {n - 1}; not measured")
    else:
        j = min(js, key=lambda j: abs(j + 1 - n // 2))
        fns = {"plain, all steps": lambda: g.generate_beam_search(start, n, prefix, **gk),
               "eos, early exit": lambda: g.generate_beam_search(start, n, prefix, eos_token_id=chain[j], **gk)}
        ts = {name: [] for name in fns}
        for fn in fns.values():
            fn()
        for _ in range(a.repeats):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append(time.perf_counter() - t0)
        print(f"early exit (topk = W = {W}, the end-of-text id is the chain's token {j + 1} of {n}; ran {g.last_steps} steps): "
              + ", ".join(f"{name} {statistics.median(v) * 1e3:.2f} ms" for name, v in ts.items()), flush=True)
    # ---- (4) the walk through the logs: host against device, 3 sentences
    S = 3
    st = K.BeamState("cuda", W, n, 64, seed=list(range(S)), groups=S, eos=never)
    st.parent_log.copy_(torch.randint(0, W, tuple(st.parent_log.shape), dtype=torch.int32))
    st.tok_log.copy_(torch.randint(0, 50257, tuple(st.tok_log.shape)))
    st.scores.copy_(-torch.rand(S * W))
    st.step.fill_(n)
    st.len.fill_(n)
    prompts = torch.full((S, 1), 50256, dtype=torch.int64, device="cuda")

    def host_walk():
        parents, toks, scores = st.parent_log.cpu().tolist(), st.tok_log.cpu().tolist(), st.scores.cpu().view(S, W)
        pr, out = prompts.cpu().tolist(), []
        for s in range(S):
            beams = []
            for b in range(W):
                seq = []
                for t in range(n - 1, -1, -1):
                    seq.append(toks[t][s * W + b])
                    b = parents[t][s * W + b]
                beams.append(pr[s] + seq[::-1])
            out.append(beams[int(scores[s].argmax())])
        return out

    def device_walk():
        ids = torch.empty((S, W, 1 + n), dtype=torch.int64, device="cuda")
        ids[:, :, :1] = prompts[:, None, :]
        scores, lens = K.beam_backtrack(st, ids, 1, never)
        return ids.cpu().tolist(), scores.cpu().tolist(), lens.cpu().tolist()

    for name, fn in (("host walk", host_walk), ("fk_beam_backtrack", device_walk)):
        fn()
        ts = []
        for _ in range(max(a.repeats, 20)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        print(f"backtrack of {S} sentences x {W} beams x {n} steps, {name:18s}: {statistics.median(ts) * 1e6:8.1f} us [{min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f}]")


def top_p_bench(g, a, prefix, start):
    """--top-p P: what the nucleus crop costs a decode step.  generate() as a hipGraph in one process, the repeats of the modes interleaved:
    greedy (top_k = 1, the figure of every other table), sampling without a crop and behind top_k = 10 (Franky.generate's default), each
    with and without top_p = P.  A random-weight decoder's distribution is nearly flat, so without a top-k crop top_p keeps most of the
    vocabulary and every logit adds its mass to the histograms: the expensive end of the mass select.  us/token is marginal like the
    default mode's, the whole call is listed with its range.  With --top-k K (0: no crop) only that crop runs, with and without top_p: under
    rocprofv3 each instantiation of the sampling kernel then has one mode's launches."""
    n, n4, B = a.new_tokens, max(1, a.new_tokens // 4), start.shape[0]
    kw = dict(prefix=prefix, use_cache=True, use_graph=True)
    modes = {} if a.top_k is not None else {"top_k = 1 (greedy)": dict(top_k=1)}
    for k in ((0, 10) if a.top_k is None else (a.top_k,)):
        name = f"top_k = {k}" if k else "no crop"
        modes[name] = dict(top_k=k or None)
        modes[f"{name}, top_p = {a.top_p}"] = dict(top_k=k or None, top_p=a.top_p)
    times = {name: {n4: [], n: []} for name in modes}
    for extra in modes.values():                            # warm up both lengths of every mode
        for k in (n4, n):
            g.generate(start, k, **kw, **extra)
    for _ in range(a.repeats):
        for k in (n4, n):
            for name, extra in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.generate(start, k, **kw, **extra)
                torch.cuda.synchronize()
                times[name][k].append(time.perf_counter() - t0)
    for name in modes:
        t4, t = statistics.median(times[name][n4]), statistics.median(times[name][n])
        step = (t - t4) / (n - n4) if n > n4 else t / n
        print(f"{name:28s}: {step * 1e6:9.1f} us/token (marginal)  {B / step:9.0f} tokens/s   | whole call {t * 1e3:8.2f} ms [{min(times[name][n]) * 1e3:.2f} .. "
              f"{max(times[name][n]) * 1e3:.2f}]", flush=True)


def rules_bench(g, a, prefix, start):
    """--repetition-penalty / --no-repeat-ngram / --min-new-tokens: what the history rules (one more launch per step, fk_logit_rules) cost a
    decode step.  generate() (top_k = 1), or with --beam W generate_beam_search on the caches, as a hipGraph in one process, the repeats of the
    modes interleaved: rules off; with --min-new-tokens (which needs an end-of-text id) the same call with that id alone, an id a
    random-weight decoder is unlikely to draw (a call that does draw it and ends early fails the run: its time would not be a step's); and the
    rules on.  us/step is marginal like every other figure of this file."""
    n, n4, B = a.new_tokens, max(1, a.new_tokens // 4), start.shape[0]
    rules = dict(repetition_penalty=a.repetition_penalty, no_repeat_ngram_size=a.no_repeat_ngram, min_new_tokens=a.min_new_tokens)
    eos = dict(eos_token_id=50255) if a.min_new_tokens > 0 else {}

    def call(k, kw):
        if a.beam:
            g.generate_beam_search(start, k, prefix, topk=a.topk, beam_width=a.beam, use_cache=True, use_graph=True, **kw)
        else:
            g.generate(start, k, prefix=prefix, top_k=1, use_cache=True, use_graph=True, **kw)
        # a call that carries the id may end early, and the marginal figure of two calls of different lengths would then mean nothing
        assert "eos_token_id" not in kw or g.last_steps == k, f"the decoder emitted the end-of-text id {kw['eos_token_id']}: {g.last_steps} of {k} steps ran; not a timing"

    modes = {"rules off": {}}
    if eos:
        modes["end-of-text id only"] = eos
    modes["rules on"] = dict(rules, **eos)
    times = {name: {n4: [], n: []} for name in modes}
    for kw in modes.values():                               # warm up both lengths of every mode
        for k in (n4, n):
            call(k, kw)
    for _ in range(a.repeats):
        for k in (n4, n):
            for name, kw in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(k, kw)
                torch.cuda.synchronize()
                times[name][k].append(time.perf_counter() - t0)
    for name in modes:
        t4, t = statistics.median(times[name][n4]), statistics.median(times[name][n])
        step = (t - t4) / (n - n4) if n > n4 else t / n
        print(f"{name:20s}: {step * 1e6:9.1f} us/step (marginal)  {B / step:9.0f} tokens/s   | whole call {t * 1e3:8.2f} ms [{min(times[name][n]) * 1e3:.2f} .. "
              f"{max(times[name][n]) * 1e3:.2f}]", flush=True)


def ctc_bench(g, a, d_model):
    """--beam W --ctc-weight L [--sentences S[,S..]]: what the CTC prefix scorer (one more launch per step, fk_ctc_prefix_score) costs the
    cached search.  CTC frames [S, --ctc-frames, 50258] of random fp32 logits, the blank last; the same call with the scorer off and on, as
    a hipGraph, in one process with the repeats interleaved; us/step is marginal like every other figure of this file.  Below them the
    launch on its own: device events around a run of back-to-back launches on a state one step into a search (it advances and scores)."""
    from frankenstein_amd import kernels as K
    W, n, n4 = a.beam, a.new_tokens, max(1, a.new_tokens // 4)
    for S in (a.sentences or [1]):
        prefix = torch.randn(S, 32, d_model, device="cuda")
        start = torch.full((S, 1), 50256, dtype=torch.long, device="cuda")
        frames = torch.randn(S, a.ctc_frames, 50258, device="cuda")
        kw = dict(topk=a.topk, beam_width=W, use_cache=True, use_graph=True)
        modes = {"scorer off": {}, f"ctc_weight = {a.ctc_weight}": dict(ctc_logits=frames, ctc_weight=a.ctc_weight, ctc_from_prompt=1)}
        times = {name: {n4: [], n: []} for name in modes}
        for extra in modes.values():                        # warm up both lengths of every mode
            for k in (n4, n):
                g.generate_beam_search(start, k, prefix, **kw, **extra)
        for _ in range(a.repeats):
            for k in (n4, n):
                for name, extra in modes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    g.generate_beam_search(start, k, prefix, **kw, **extra)
                    torch.cuda.synchronize()
                    times[name][k].append(time.perf_counter() - t0)
        for name in modes:
            t4, t = statistics.median(times[name][n4]), statistics.median(times[name][n])
            step = (t - t4) / (n - n4) if n > n4 else t / n
            print(f"S = {S:2d}  {name:20s}: {step * 1e6:9.1f} us/step (marginal)   | whole call {t * 1e3:8.2f} ms [{min(times[name][n]) * 1e3:.2f} .. "
                  f"{max(times[name][n]) * 1e3:.2f}], {n4} tokens {t4 * 1e3:8.2f} ms", flush=True)
        # the launch on its own: row r continues beam r % W with a token of the vocabulary, then scores topk candidates
        cs = K.ctc_prefix_init(frames, W, a.ctc_weight, None, None, start)
        st = K.BeamState("cuda", W, 2, 64, seed=list(range(S)), groups=S)
        st.parent_log[0] = (torch.arange(S * W, device="cuda") % W).to(torch.int32)
        st.tok_log[0] = torch.randint(0, 50256, (S * W,), device="cuda")
        st.step.fill_(1)
        top_id = torch.stack([torch.randperm(50257, device="cuda")[:a.topk] for _ in range(S * W)])
        top_lp = torch.full((S * W, a.topk), -3.0, device="cuda")
        reps = 200
        for _ in range(20):
            K.ctc_prefix_score_(top_lp, top_id, cs, st)
        ts = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                K.ctc_prefix_score_(top_lp, top_id, cs, st)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / reps)
        print(f"S = {S:2d}  fk_ctc_prefix_score alone ({S * W} rows x {a.topk} candidates x {a.ctc_frames} frames): {statistics.median(ts):7.2f} us per launch, "
              f"back to back [{min(ts):.2f} .. {max(ts):.2f}]", flush=True)


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
    ap.add_argument("--eos", action="store_true", help="with --beam: the end-of-text path (step against the plain step, cost of the poll, early exit, backtrack)")
    ap.add_argument("--top-p", type=float, default=None, help="nucleus sampling: time generate with and without top_p = P (greedy, no crop, top_k = 10), interleaved")
    ap.add_argument("--top-k", type=int, default=None, help="with --top-p: only this top-k crop (0: none), with and without top_p")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, help="history rules: time generate (or, with --beam, the cached search) with and without them, interleaved")
    ap.add_argument("--no-repeat-ngram", type=int, default=0, help="history rules: no_repeat_ngram_size")
    ap.add_argument("--min-new-tokens", type=int, default=0, help="history rules: min_new_tokens (the calls then carry an end-of-text id)")
    ap.add_argument("--ctc-weight", type=float, default=None, help="with --beam: joint CTC / attention decoding, the search with and without the prefix scorer")
    ap.add_argument("--ctc-frames", type=int, default=32, help="with --ctc-weight: frames of the CTC head")
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
    if a.repetition_penalty != 1.0 or a.no_repeat_ngram or a.min_new_tokens:
        if a.beam and B != 1:
            ap.error("--beam with --batch: one sentence only")
        print(f"history rules: repetition_penalty {a.repetition_penalty}, no_repeat_ngram_size {a.no_repeat_ngram}, min_new_tokens {a.min_new_tokens}"
              + (f"; beam width {a.beam}, topk {a.topk}" if a.beam else ""))
        return rules_bench(g, a, prefix, start)
    if a.ctc_weight is not None:
        if not a.beam or B != 1:
            ap.error("--ctc-weight needs --beam (and --sentences for more than one sentence)")
        print(f"beam width {a.beam}, topk {a.topk}, CTC prefix scorer with weight {a.ctc_weight} on {a.ctc_frames} frames")
        return ctc_bench(g, a, m["n_embd"])
    if a.beam and a.sentences:
        print(f"beam width {a.beam}, topk {a.topk}, sentences {a.sentences}")
        return sentences_bench(g, a, m["n_embd"])
    if a.beam:
        if B != 1:
            ap.error("--beam with --batch: give the number of sentences as --sentences")
        if a.eos:
            print(f"beam width {a.beam}, topk {a.topk}, end-of-text")
            return eos_bench(g, a, prefix, start)
        print(f"beam width {a.beam}, topk {a.topk}")
        return beam_bench(g, a, prefix, start)
    if a.top_p is not None:
        print(f"nucleus sampling, top_p = {a.top_p}")
        return top_p_bench(g, a, prefix, start)
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
