#!/usr/bin/env python
"""Times of the signal augmentation on one MI355X at (B 32, T 600, C 256, P 25, ldp 32, bf16) and (B 32, T 768, C 256, P 32, ldp 32, bf16):

  * fk_patchify (the yardstick: the parent's launch at the same shape);
  * fk_augment_patchify with noise only, with masks only (drop, spans, shift) and with everything on;
  * the signal mode (P = 1, fp32), the extra pass a model with a DayAdapter pays;
  * the composition a user writes today: torch.randn_like + adds + mask multiplies, then fk_patchify;
  * the whole brainformer-small training step with the augmentation off and on, in this one process, in interleaved rounds.

Kernels are timed with HIP events around `reps` back-to-back launches, in interleaved rounds; median and minimum over the rounds are
printed.  Floors: the traffic (x read once, tokens written once) at 5 TB/s, and the Philox blocks the launch computes.
Usage: python tools/augment_bench.py [--rounds 7] [--reps 20] [--steps 6] [--out FILE.md]"""
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
    g = torch.Generator(device=dev).manual_seed(1)
    words = E.augment_words(dev)
    noise = E.AugmentConfig(white_sd=0.5, offset_sd=0.3)
    masks = E.AugmentConfig(chan_drop_p=0.1, time_shift=8, n_time_masks=4, time_mask_len=40)
    full = E.AugmentConfig(white_sd=0.5, offset_sd=0.3, chan_drop_p=0.1, time_shift=8, n_time_masks=4, time_mask_len=40)
    lines = []
    for B, T, C, P, kp in ((32, 600, 256, 25, 32), (32, 768, 256, 32, 32)):
        x = torch.randn(B, T, C, device=dev, generator=g)
        x[:, T - 40:] = 0.0                                          # a padded tail, as the input pipeline leaves it

        def torch_composition():
            n = torch.randn_like(x)
            off = torch.randn(B, 1, C, device=dev) * 0.3
            keep = (torch.rand(B, 1, C, device=dev) >= 0.1).float()
            tm = torch.ones(B, T, 1, device=dev)
            tm[:, 100:140] = 0.0                                     # one span; drawing four per sample would cost a torch user more
            valid = (x != 0).any(dim=2, keepdim=True).float()
            y = (x + (0.5 * n + off) * valid) * keep * tm
            return K.patchify(y, P, kp, torch.bfloat16)

        arms = {"fk_patchify": lambda: K.patchify(x, P, kp, torch.bfloat16),
                "fk_augment_patchify, all knobs zero": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, E.AugmentConfig(), words),
                "fk_augment_patchify, noise only": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, noise, words),
                "fk_augment_patchify, masks only": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, masks, words),
                "fk_augment_patchify, white noise alone (keep_padding off)": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, E.AugmentConfig(white_sd=0.5, keep_padding=False), words),
                "fk_augment_patchify, offset alone (keep_padding off)": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, E.AugmentConfig(offset_sd=0.3, keep_padding=False), words),
                "fk_augment_patchify, shift alone": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, E.AugmentConfig(time_shift=8), words),
                "fk_augment_patchify, 4 spans alone": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, E.AugmentConfig(n_time_masks=4, time_mask_len=40), words),
                "fk_augment_patchify, electrode drop alone": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, E.AugmentConfig(chan_drop_p=0.1), words),
                "fk_augment_patchify, everything": lambda: K.augment_patchify(x, P, kp, torch.bfloat16, full, words),
                "signal mode (P = 1, fp32), everything": lambda: K.augment_patchify(x, 1, 1, torch.float32, full, words),
                "torch composition + fk_patchify": torch_composition}
        for fn in arms.values():
            timed(fn, 3)
        res = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                res[k].append(timed(fn, args.reps))
        base = statistics.median(res["fk_patchify"])
        nbytes = x.numel() * 4 + B * (T // P) * C * kp * 2
        blocks = B * T * (C // 4)
        lines += [f"B {B}, T {T}, C {C}, P {P}, ldp {kp}, bf16: {nbytes / 1e6:.1f} MB of traffic ({nbytes / 5.0e12 * 1e6:.1f} us at 5 TB/s), "
                  f"{blocks / 1e6:.2f} M white-noise Philox blocks", "",
                  "| launch | median us | min us | / fk_patchify | achieved GB/s |", "|---|---|---|---|---|"]
        for k, v in res.items():
            med = statistics.median(v)
            nb = x.numel() * 8 if "signal" in k else nbytes
            lines.append(f"| {k} | {med:.1f} | {min(v):.1f} | {med / base:.2f} | {'-' if 'torch' in k else '%.0f' % (nb / med / 1e3)} |")
        lines.append("")

    # the whole training step, augmentation off against on, interleaved
    B, T, C = 32, 600, 256
    x = torch.randn(B, T, C, device=dev, generator=g)
    y = torch.randn(B, 32, 128, device=dev, generator=g)

    def build(**aug):
        enc = bf.MAEConfig(window_size=600, n_electrodes=256, patch_size=25, dim=384, n_layers=6, head_dim=64, hidden_dim=1536, n_heads=6,
                           n_kv_heads=6, **aug)
        cfg = bf.Config(encoder=enc, n_output_tokens=32, output_dim=128, dim=384, n_layers=2, head_dim=64, hidden_dim=768, n_heads=6, n_kv_heads=6)
        m = bf.BrainFormer(cfg)
        bench.init_weights(m)
        m.to(dev)
        tcfg = tu.TrainConfig(batch_size=B, mixed_precision=True, use_scheduler=False, learning_rate=1e-4)
        opt = tu.FusedAdamW(m, lr=tcfg.learning_rate, weight_decay=tcfg.weight_decay, grad_clip=tcfg.grad_clip)
        return m, opt, tcfg, tu.init_lr_scheduler(tcfg)

    runs = {"augmentation off": build(),
            "augmentation on (everything)": build(aug_white_sd=0.5, aug_offset_sd=0.3, aug_chan_drop=0.1, aug_time_shift=8, aug_time_masks=4,
                                                  aug_time_mask_len=40)}
    step_ms = {k: [] for k in runs}
    counters = {k: 0 for k in runs}

    def steps(k, n):
        m, opt, tcfg, sched = runs[k]
        for _ in range(n):
            tu.train_step(m, (x, y, None), opt, counters[k], tcfg, sched)
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
    base = statistics.median(step_ms["augmentation off"])
    lines += ["| training step (brainformer-small, B = 32, bf16) | median ms | min ms | difference | ratio |", "|---|---|---|---|---|"]
    for k, v in step_ms.items():
        med = statistics.median(v)
        lines.append(f"| {k} | {med:.2f} | {min(v):.2f} | {med - base:+.2f} ms | {med / base:.4f} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
