#!/usr/bin/env python
"""Times of the low-rank adapter kernels and of an adapted Franky step on one MI355X.

Kernels (csrc/lora.hip), M = 1824 rows (32 x 57), r = 16, bf16, at the four GPT-2 124M Linears (c_attn 768 -> 2304, attention c_proj
768 -> 768, c_fc 768 -> 3072, MLP c_proj 3072 -> 768): fk_lora_fwd (in place on a residual), the same entry point in the data-gradient role,
fk_lora_wgrad, and the torch composition of the same products (`res + s * ((x @ A.T) @ B.T)`; `s * dy.T @ u` and `s * du.T @ x`), timed
with HIP events around `reps` back-to-back launches in interleaved rounds; median and minimum over the rounds.  Floors are the bytes
each call must move (x or dy once, the output read and written once, u once) at 5 TB/s.

Steps: Franky = BrainEncoder(Config(MAEConfig(window_size=768, patch_size=32), output_dim=768)) + a randomly initialised GPT-2 124M,
B = 32, 25 tokens, bf16, train_step with FusedAdamW, in three configurations in this one process, in interleaved rounds: full fine-tune,
frozen decoder, LoRA r = 16 on all four targets.  For each: optimizer-state bytes (both moment arenas) and bytes all-reduced per step
under data parallel (the gradient arena).  `--configs full` times the full fine-tune alone (what an older checkout can run too).
Usage: python tools/lora_bench.py [--rounds 7] [--reps 20] [--steps 6] [--configs full,frozen,lora] [--no-kernels] [--out FILE.md]"""
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


def kernel_table(args, lines):
    from frankenstein_amd import kernels as K
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    M, r, s = 1824, 16, 2.0
    bf = torch.bfloat16
    shapes = {"c_attn": (768, 2304), "attn.c_proj": (768, 768), "c_fc": (768, 3072), "mlp.c_proj": (3072, 768)}
    arms, floors = {}, {}
    for name, (Kd, N) in shapes.items():
        x = torch.randn(M, Kd, device=dev, generator=g).to(bf)
        dy = torch.randn(M, N, device=dev, generator=g).to(bf)
        A = (torch.randn(r, Kd, device=dev, generator=g) / Kd ** 0.5).to(bf)
        Bm = torch.randn(N, r, device=dev, generator=g).to(bf)
        At, Bt = A.t().contiguous(), Bm.t().contiguous()
        y = torch.randn(M, N, device=dev, generator=g).to(bf)
        dh = torch.randn(M, Kd, device=dev, generator=g).to(bf)
        _, u = K.lora_fwd(x, A, Bm, s, res=y, out=y)
        _, du = K.lora_fwd(dy, Bt, At, s, res=dh, out=dh)
        dA, dB = K.lora_wgrad(dy, u, du, x, s)
        arms[f"{name}: fk_lora_fwd"] = lambda x=x, A=A, Bm=Bm, y=y: K.lora_fwd(x, A, Bm, s, res=y, out=y)
        arms[f"{name}: torch forward"] = lambda x=x, A=A, Bm=Bm, y=y: y.add_((x @ A.t()) @ Bm.t(), alpha=s)
        arms[f"{name}: fk_lora_fwd (data gradient)"] = lambda dy=dy, At=At, Bt=Bt, dh=dh: K.lora_fwd(dy, Bt, At, s, res=dh, out=dh)
        arms[f"{name}: torch data gradient"] = lambda dy=dy, A=A, Bm=Bm, dh=dh: dh.add_((dy @ Bm) @ A, alpha=s)
        arms[f"{name}: fk_lora_wgrad"] = lambda dy=dy, u=u, du=du, x=x, dA=dA, dB=dB: K.lora_wgrad(dy, u, du, x, s, dA=dA, dB=dB, accumulate=True)
        arms[f"{name}: torch weight gradients"] = lambda dy=dy, u=u, du=du, x=x, dA=dA, dB=dB: (
            dB.add_(dy.t().float() @ u.float(), alpha=s), dA.add_(du.t().float() @ x.float(), alpha=s))
        floors[f"{name}: fk_lora_fwd"] = 2 * (M * Kd + 2 * M * N + M * r)
        floors[f"{name}: fk_lora_fwd (data gradient)"] = 2 * (M * N + 2 * M * Kd + M * r)
        floors[f"{name}: fk_lora_wgrad"] = 2 * (M * N + M * Kd + 2 * M * r) + 8 * (N * r + r * Kd)
    for fn in arms.values():
        timed(fn, 3)
    res = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, args.reps))
    lines += [f"Kernels, M = {M}, r = {r}, bf16, {args.reps} back-to-back launches x {args.rounds} interleaved rounds:", "",
              "| call | median us | min us | bytes floor us (5 TB/s) |", "|---|---|---|---|"]
    for k, v in res.items():
        fl = floors.get(k)
        lines.append(f"| {k} | {statistics.median(v):.1f} | {min(v):.1f} | {'%.1f' % (fl / 5.0e12 * 1e6) if fl else '-'} |")
    lines.append("")


def build(kind):
    import bench
    from frankenstein_amd.models import brainformer as bf, gpt2_model as g2
    from frankenstein_amd.models.notebook_models import BrainEncoder, Franky
    from frankenstein_amd.utils import train_utils as tu
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    enc = bf.MAEConfig(window_size=768, patch_size=32)
    brain = BrainEncoder(bf.Config(encoder=enc, output_dim=768))
    gpt = g2.GPT(g2.GPTConfig(block_size=1024, vocab_size=50257, n_layer=12, n_head=12, n_embd=768, dropout=0.0, bias=True))
    fr = Franky(brain, gpt)
    bench.init_weights(fr.brain_model)
    fr.to(dev)
    if kind == "frozen":
        for p in gpt.parameters():
            p.requires_grad_(False)
    elif kind == "lora":
        gpt.add_lora(rank=16, alpha=32.0)
        with torch.no_grad():
            for k, p in gpt.lora_state_dict().items():
                if k.endswith("lora_B"):
                    p.normal_(0.0, 0.02)
    tcfg = tu.TrainConfig(batch_size=32, mixed_precision=True, use_scheduler=False, learning_rate=1e-4)
    opt = tu.FusedAdamW(fr, lr=tcfg.learning_rate, weight_decay=tcfg.weight_decay, grad_clip=tcfg.grad_clip)
    return fr, opt, tcfg, tu.init_lr_scheduler(tcfg)


def step_table(args, lines):
    from frankenstein_amd.utils import train_utils as tu
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(32, 768, 256, device=dev, generator=g)
    tok = torch.randint(0, 50256, (32, 25), device=dev, generator=g)
    names = {"full": "full fine-tune", "frozen": "frozen decoder", "lora": "LoRA r = 16"}
    runs = {k: build(k) for k in args.configs.split(",")}
    counters = {k: 0 for k in runs}
    step_ms = {k: [] for k in runs}

    def steps(k, n):
        fr, opt, tcfg, sched = runs[k]
        for _ in range(n):
            tu.train_step(fr, (x, tok, None), opt, counters[k], tcfg, sched)
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
    lines += [f"Franky step (B = 32, 25 tokens, bf16), {args.steps} steps x {args.rounds} interleaved rounds:", "",
              "| configuration | median ms | min ms | trainable parameters | optimizer state MB | all-reduced per step MB |", "|---|---|---|---|---|---|"]
    for k, v in step_ms.items():
        opt = runs[k][1]
        n = sum(p.numel() for p in opt.arena.params)
        lines.append(f"| {names[k]} | {statistics.median(v):.2f} | {min(v):.2f} | {n / 1e6:.2f} M | {(opt.m.numel() + opt.v.numel()) * 4 / 1e6:.1f} | "
                     f"{opt.arena.grad.numel() * 4 / 1e6:.1f} |")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--configs", default="full,frozen,lora")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X: there is no CPU timing"
    import frankenstein_amd as fa
    fa.set_compute_dtype("bf16")
    lines = []
    if not args.no_kernels:
        kernel_table(args, lines)
    step_table(args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
