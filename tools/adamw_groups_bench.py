"""Times the optimizer kernels on a GPT-2-124M-sized arena (profiles/adamw_groups.md):
  fk_adamw_step         one launch over the whole arena (the one-group optimizer)
  fk_adamw_step_groups  the same arena through the decay / no-decay segment table of GPT.configure_optimizers, and through a
                        one-segment table (the lookup's own cost)
  fk_grad_sumsq         the squared gradient norm over the same table
Device events around `iters` back-to-back launches, the variants alternated over `rounds` rounds; prints and returns the median
microseconds per launch and the bytes each kernel has to move.  python tools/adamw_groups_bench.py [out.json]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from frankenstein_amd import kernels as K                                   # noqa: E402
from frankenstein_amd.models import gpt2_model as g2                        # noqa: E402
from frankenstein_amd.utils import train_utils as tu                        # noqa: E402


def gpt2_124m_tables():
    """arena size and the one launch's table for GPT-2 124M with the reference's two groups, every parameter reached"""
    g = g2.GPT(g2.GPTConfig(block_size=1024, vocab_size=50257, n_layer=12, n_head=12, n_embd=768, dropout=0.0, bias=True))
    params = tu._unique_trainable(g)
    group_of = [0 if p.dim() >= 2 else 1 for p in params]
    sizes = [p.numel() for p in params]
    offsets, off = [], 0
    for n in sizes:
        offsets.append(off)
        off += (n + 3) // 4 * 4
    (segs, slots), = tu.adamw_tables(offsets, sizes, group_of, [True] * len(params), None, 1)
    return off, segs, slots, len(params)


def main(out=None, iters=20, rounds=5):
    assert torch.cuda.is_available()
    n, segs, slots, nparams = gpt2_124m_tables()
    dev = torch.device("cuda")
    p, m = torch.randn(n, device=dev), torch.zeros(n, device=dev)
    g, v = torch.randn(n, device=dev) * 0.1, torch.zeros(n, device=dev)
    table, one = K.adamw_segments(segs, dev), K.adamw_segments([(0, n, 0)], dev)
    hyper = [(3e-4, 0.9, 0.95, 1e-8, 0.1 if gi == 0 else 0.0, 10) for gi, _ in slots]
    partials, norm = torch.empty(K.GRAD_SUMSQ_BLOCKS, device=dev), torch.zeros(1, device=dev)
    K.grad_sumsq_(g, table, partials)
    variants = {
        "fk_adamw_step": lambda: K.adamw_step_(p, g, m, v, 10, 3e-4, 0.9, 0.95, 1e-8, 0.1, clip=1.0, zero_grad=True),
        "fk_adamw_step_groups(decay table)": lambda: K.adamw_step_groups_(p, g, m, v, table, hyper, clip=1.0, zero_grad=True),
        "fk_adamw_step_groups(one segment)": lambda: K.adamw_step_groups_(p, g, m, v, one, hyper[:1], clip=1.0, zero_grad=True),
        "fk_adamw_step_groups(decay table, max_norm)": lambda: K.adamw_step_groups_(p, g, m, v, table, hyper, zero_grad=True, max_norm=1.0,
                                                                                    partials=partials, norm_out=norm),
        "fk_grad_sumsq": lambda: K.grad_sumsq_(g, table, partials),
    }
    times = {k: [] for k in variants}
    for f in variants.values():                              # warm-up: code objects, clocks
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / iters)
    covered = sum(e - b for b, e, _ in segs)
    res = {"arena_elements": n, "parameters": nparams, "segments": len(segs), "slots": len(slots), "covered_elements": covered,
           "iters": iters, "rounds": rounds, "us_per_launch": {}}
    for name, ts in times.items():
        nbytes = 4 * covered * (1 if name == "fk_grad_sumsq" else 8)         # step: read p g m v, write p m v and the zeroed g
        med = statistics.median(ts)
        res["us_per_launch"][name] = {"median": round(med, 1), "min": round(min(ts), 1), "max": round(max(ts), 1),
                                      "GB_per_s": round(nbytes / med / 1e3, 1)}
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
