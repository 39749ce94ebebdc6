#!/usr/bin/env python3
"""Generate tests/golden/gpt2_124m_generate.npz by RUNNING THE REFERENCE (CPU, fp32): greedy decoding of the reference's GPT
(models/gpt2_model.py:328-353) at its real decoder size, GPT-2 124M (d = 768, 12 layers, 12 heads, V = 50257), synthetic weights.

Same recipe as make_golden.py (whose stubs and load_synth are imported, not restated): the reference's own modules are imported
from the mounted reference tree, nothing of it is copied; only OUTPUT numbers are stored.  The [8, 50257] step logits would be
1.6 MB, so each step keeps what a decode test needs: the log-sum-exp, the 64 largest logits with their ids, and every 97th column.

The greedy tokens are only a fair target when the reference itself is decisive: every step's top-1 / top-2 logit gap must be at
least MIN_GAP = 1e-3, ten times the 1e-4 logit tolerance of the fp32 decode tests.  If a prefix seed gives a closer call the next
seed of PREFIX_SEEDS is tried; the seed used is recorded in the file.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_decode.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, str(Path(__file__).resolve().parent))

import make_golden as MG  # noqa: E402
from frankenstein_amd import synth  # noqa: E402

PREFIX_SEEDS = (99, 100, 101, 102, 103)
MIN_GAP = 1e-3
NEW_TOKENS, T_PREFIX, START = 8, 32, 50256
COL_STRIDE, TOPN = 97, 64


def run(g, seed):
    prefix = torch.from_numpy(synth.make_motion_targets(1, T_PREFIX, 768, seed=seed))
    start = torch.full((1, 1), START, dtype=torch.int64)
    gen = g.generate(start.clone(), max_new_tokens=NEW_TOKENS, prefix=prefix, top_k=1)
    cur, steps = start.clone(), []
    for _ in range(NEW_TOKENS):
        _, lg = g(cur, prefix=prefix)
        steps.append(lg[0, -1].detach().double())
        cur = torch.cat([cur, lg[:, -1].argmax(-1, keepdim=True)], 1)
    assert cur[0].tolist() == gen.reshape(-1).tolist(), "generate(top_k=1) is the arg-max chain"
    lg = torch.stack(steps)                                         # [8, V] float64 copies of the fp32 logits
    top_v, top_i = lg.topk(TOPN, dim=-1)
    gap = float((top_v[:, 0] - top_v[:, 1]).min())
    return dict(seed=np.array(seed), start=start.numpy(), tokens=gen.reshape(-1).numpy(), lse=torch.logsumexp(lg, -1).numpy(),
                top_ids=top_i.numpy(), top_vals=top_v.float().numpy(), cols=lg[:, ::COL_STRIDE].float().numpy(),
                col_stride=np.array(COL_STRIDE), min_gap=np.array(gap)), gap


def main():
    _, g2, _ = MG.import_reference()
    torch.manual_seed(0)
    g = g2.GPT(g2.GPTConfig(block_size=1024, vocab_size=50257, n_layer=12, n_head=12, n_embd=768, dropout=0.0, bias=True)).float()
    MG.load_synth(g)
    g.eval()
    with torch.no_grad():
        for seed in PREFIX_SEEDS:
            arrs, gap = run(g, seed)
            print(f"prefix seed {seed}: smallest top-1/top-2 gap {gap:.3e}")
            if gap >= MIN_GAP:
                break
        else:
            raise SystemExit("no prefix seed of the list gives a decisive greedy chain")
    MG.save("gpt2_124m_generate", **arrs)


if __name__ == "__main__":
    main()
