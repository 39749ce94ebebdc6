#!/usr/bin/env python
"""Times of the per-session input adapter on one MI355X at the benchmarked size (B = 32, T = 600, C = 256, P = 25, n_days = 24, bf16):

  * fk_day_adapter_fwd beside fk_patchify alone;
  * the backward: the d_tok GEMM (dh @ emb_w, fp32 out) plus fk_day_adapter_bwd;
  * both with one day for the whole batch and with 24 distinct days;
  * the whole brainformer-small training step with n_days = 24 against n_days = 0, in this one process, in interleaved rounds.

Kernels are timed with HIP events around `reps` back-to-back launches, in interleaved rounds; median and minimum over the rounds are
printed.  Floors: the forward and the weight gradient are 2 * B * T * C * C FLOP each on the exact fp32-input MFMA, for which an untuned
tiled kernel reaches about 120 TFLOP/s (the yardstick of csrc/dayadapt.hip's header); the forward also reads x once and writes the tokens
once.  Usage: python tools/day_adapter_bench.py [--rounds 7] [--reps 20] [--steps 6] [--out FILE.md]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import frankenstein_amd as fa
    from frankenstein_amd import engine as E, kernels as K
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype("bf16")
    dev = torch.device("cuda", 0)
    B, T, C, P, ND, d = 32, 600, 256, 25, 24, 384
    kp, nT = 32, T // P
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, T, C, device=dev, generator=g)
    delta = torch.randn(ND, C, C, device=dev, generator=g) / 16
    bias = torch.randn(ND, C, device=dev, generator=g)
    dh = torch.randn(B * nT * C, d, device=dev, generator=g).bfloat16()
    emb_w = torch.nn.Parameter(torch.randn(d, P, device=dev, generator=g) / 5)
    days = {"one day": torch.full((B,), 7, device=dev), "24 days": torch.arange(B, device=dev) % ND}
    d_tok = E._d_tok(dh, emb_w, kp)
    arms = {"fk_patchify": lambda: K.patchify(x, P, kp, torch.bfloat16),
            "d_tok GEMM": lambda: E._d_tok(dh, emb_w, kp)}
    for name, day in days.items():
        arms[f"fk_day_adapter_fwd, {name}"] = lambda day=day: K.day_adapter_fwd(x, day, delta, bias, P, kp, torch.bfloat16)
        arms[f"fk_day_adapter_bwd, {name}"] = lambda day=day: K.day_adapter_bwd(x, day, d_tok, P, delta.shape)
    for fn in arms.values():
        timed(fn, 3)
    res = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, args.reps))
    flop = 2.0 * B * T * C * C
    floor_mfma = flop / 120e12 * 1e6
    lines = ["| kernel | median us | min us | floor us | median / floor |", "|---|---|---|---|---|"]
    for k, v in res.items():
        fl = floor_mfma if "day_adapter" in k else None
        med = statistics.median(v)
        lines.append(f"| {k} | {med:.1f} | {min(v):.1f} | {'%.1f' % fl if fl else '-'} | {'%.1f' % (med / fl) if fl else '-'} |")
    io_us = (x.numel() * 4 + B * nT * C * kp * 2) / 5.0e12 * 1e6
    lines.append("")
    lines.append(f"MFMA floor {floor_mfma:.1f} us = {flop / 1e9:.2f} GFLOP at 120 TFLOP/s; the forward's traffic (x once, tokens once, "
                 f"{(x.numel() * 4 + B * nT * C * kp * 2) / 1e6:.1f} MB) is {io_us:.1f} us at 5 TB/s.")

    # the whole training step, n_days = 24 against n_days = 0, interleaved
    def build(n_days):
        enc = bf.MAEConfig(window_size=600, n_electrodes=256, patch_size=25, dim=384, n_layers=6, head_dim=64, hidden_dim=1536, n_heads=6,
                           n_kv_heads=6, n_days=n_days)
        cfg = bf.Config(encoder=enc, n_output_tokens=32, output_dim=128, dim=384, n_layers=2, head_dim=64, hidden_dim=768, n_heads=6, n_kv_heads=6)
        m = bf.BrainFormer(cfg)
        bench.init_weights(m)
        m.to(dev)
        if n_days:
            with torch.no_grad():
                m.encoder.day_adapter.delta.mul_(0.1)
                m.encoder.day_adapter.bias.mul_(0.1)
        tcfg = tu.TrainConfig(batch_size=B, mixed_precision=True, use_scheduler=False, learning_rate=1e-4)
        opt = tu.FusedAdamW(m, lr=tcfg.learning_rate, weight_decay=tcfg.weight_decay, grad_clip=tcfg.grad_clip)
        return m, opt, tcfg, tu.init_lr_scheduler(tcfg)

    y = torch.randn(B, 32, 128, device=dev, generator=g)
    runs = {"n_days = 0": (build(0), None), "n_days = 24, one day": (build(ND), days["one day"]), "n_days = 24, 24 days": (build(ND), days["24 days"])}
    step_ms = {k: [] for k in runs}
    counters = {k: 0 for k in runs}

    def steps(k, n):
        (m, opt, tcfg, sched), day = runs[k]
        for _ in range(n):
            tu.train_step(m, (x, y, day), opt, counters[k], tcfg, sched)
            counters[k] += 1

    for k in runs:
        steps(k, 3)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k in runs:
            t0 = time.perf_counter()
            steps(k, args.steps)
            torch.cuda.synchronize()
            step_ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
    base = statistics.median(step_ms["n_days = 0"])
    lines += ["", "| training step (B = 32, bf16) | median ms | min ms | difference to n_days = 0 | share of the step |", "|---|---|---|---|---|"]
    for k, v in step_ms.items():
        med = statistics.median(v)
        lines.append(f"| {k} | {med:.2f} | {min(v):.2f} | {med - base:+.2f} ms | {100 * (med - base) / base:+.2f} % |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
