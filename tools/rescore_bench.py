"""LM rescoring of CTC n-best lists, packed against flat (profiles/lm_rescore.md).

GPT-2 124M, random init, bf16.  S = 32 sentences; the hypotheses come from engine.ctc_beam_decode (W = 32, nbest = 32) on seeded peaked
logits [32, 32, 50258] and are cut to T = 25 tokens; a list of n takes the first n.  P = 0 or 32 rows of a random brain prefix.

  packed        GPT.rescore_nbest(max_nodes=None): trie, one host read that sizes the forward, packed forward, head statistics, ranking
  packed static GPT.rescore_nbest(max_nodes=N), N = what the run above chose: nothing waits for the host
  flat          what a user writes from the public calls without it: GPT.forward on [S n, 1 + T] with the prefix repeated and targets
                (the only call that returns every position's logits), log_softmax, gather, sum, the totals and a sort; chunked over
                sentences so that at most --flat-rows sequences are in flight and the logits fit

Warm-up, then --rounds rounds that alternate the sides; every call is bracketed by device synchronisation; the median is reported.
--only packed|static|flat with --n / --prefix runs one side alone (for rocprofv3 --kernel-trace --stats, which gets a run of its own).
One JSON line per configuration, then a markdown table."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import frankenstein_amd as fa                                          # noqa: E402
from frankenstein_amd import engine as E                               # noqa: E402
from frankenstein_amd.models.gpt2_model import GPT, GPTConfig          # noqa: E402

S, FRAMES, C, T, BOS = 32, 32, 50258, 25, 50256


def nbest_lists(seed=0):
    """the 32-best lists of S sentences from peaked logits: per frame the sentence's own class at +9, two rivals at +7 and +6, the blank
    at +7 on a third of the frames, over randn -> (ids [S, 32, T], lengths [S, 32], scores [S, 32])"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn((S, FRAMES, C), generator=g, device="cuda")
    pick = torch.randint(0, C - 2, (S, FRAMES, 3), generator=g, device="cuda")
    logits.scatter_add_(2, pick, torch.tensor([9.0, 7.0, 6.0], device="cuda").expand(S, FRAMES, 3).contiguous())
    blank_on = torch.rand((S, FRAMES), generator=g, device="cuda") < 0.33
    logits[:, :, C - 1] += 7.0 * blank_on
    ids, lengths, scores = E.ctc_beam_decode(logits, blank=C - 1, beam_width=32, nbest=32)
    return ids[:, :, :T].contiguous(), lengths.clamp(max=T), scores


def flat_rescore(m, ids, lengths, scores, prefix, max_rows):
    """-> (total [S, n], order [S, n]); eos = BOS behind every hypothesis, as the packed side scores it"""
    Sn, n, Tn = ids.shape
    per = max(1, max_rows // n)
    lm = torch.empty((Sn, n), dtype=torch.float32, device=ids.device)
    for s0 in range(0, Sn, per):
        tok = ids[s0:s0 + per].reshape(-1, Tn).clamp(0, BOS)
        lens = lengths[s0:s0 + per].reshape(-1)
        idx = torch.cat([torch.full((tok.shape[0], 1), BOS, dtype=torch.int64, device=ids.device), tok], dim=1)
        pf = None if prefix is None else prefix[s0:s0 + per].repeat_interleave(n, dim=0)
        _, logits = m(idx, prefix=pf, targets=idx)
        logp = torch.log_softmax(logits.float(), dim=-1)
        nxt = logp[:, :-1].gather(2, tok[:, :, None])[:, :, 0]
        keep = torch.arange(Tn, device=ids.device)[None, :] < lens[:, None]
        part = (nxt * keep).sum(1) + logp[torch.arange(tok.shape[0], device=ids.device), lens, BOS]
        lm[s0:s0 + per] = part.view(-1, n)
    total = scores + lm
    return total, torch.sort(total, dim=1, descending=True, stable=True).indices


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1, 5, 8, 32])
    ap.add_argument("--prefix", type=int, nargs="*", default=[0, 32])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flat-rows", type=int, default=256)
    ap.add_argument("--only", choices=["packed", "static", "flat"], default=None)
    args = ap.parse_args()
    fa.set_compute_dtype("bf16")
    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=1024, vocab_size=50257, n_layer=12, n_head=12, n_embd=768, bias=True)).cuda().eval()
    ids32, len32, sc32 = nbest_lists()
    rows = []
    with torch.no_grad():
        for P in args.prefix:
            g = torch.Generator(device="cuda").manual_seed(100 + P)
            prefix = torch.randn((S, P, 768), generator=g, device="cuda").to(torch.bfloat16) if P else None
            for n in args.n:
                ids, lengths, scores = ids32[:, :n].contiguous(), len32[:, :n].contiguous(), sc32[:, :n].contiguous()
                kw = dict(prefix=prefix, eos_token_id=BOS)
                _, n_nodes = m.score_nbest(ids, lengths, am_scores=scores, **kw)
                N = (P + int(n_nodes.max()) + 7) // 8 * 8 - P
                sides = {"packed": lambda: m.rescore_nbest(ids, lengths, scores, **kw),
                         "static": lambda: m.rescore_nbest(ids, lengths, scores, max_nodes=N, **kw),
                         "flat": lambda: flat_rescore(m, ids, lengths, scores, prefix, args.flat_rows)}
                if args.only:
                    sides = {args.only: sides[args.only]}
                for _ in range(args.warmup):
                    for f in sides.values():
                        f()
                ms = {k: [] for k in sides}
                for _ in range(args.rounds):
                    for k, f in sides.items():
                        ms[k].append(timed(f))
                rec = dict(n=n, P=P, S=S, T=T, N=N, nodes_mean=float(n_nodes.float().mean()), nodes_max=int(n_nodes.max()),
                           mean_len=float(lengths.float().mean()), trunk_rows_packed=S * (P + N), trunk_rows_flat=S * n * (P + 1 + T),
                           head_rows_packed=S * (N - 1 + n), head_rows_flat=S * n * (1 + T), ms={k: statistics.median(v) for k, v in ms.items()},
                           ms_min={k: min(v) for k, v in ms.items()})
                if not args.only:                                       # the two sides rank alike
                    got = m.rescore_nbest(ids, lengths, scores, **kw)
                    tot, order = flat_rescore(m, ids, lengths, scores, prefix, args.flat_rows)
                    rec["order_agree"] = float((got[5] == order).float().mean())
                    rec["max_total_diff"] = float((got[4] - tot.gather(1, got[5])).abs().max())
                rows.append(rec)
                print(json.dumps(rec), flush=True)
    print("\n| P | n | nodes / sentence (mean, max) | N | trunk rows packed / flat | head rows packed / flat | packed | packed static | flat | flat / packed |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        t = r["ms"]
        ratio = f"{t['flat'] / t['packed']:.2f}" if "flat" in t and "packed" in t else "-"
        print(f"| {r['P']} | {r['n']} | {r['nodes_mean']:.1f}, {r['nodes_max']} | {r['N']} | {r['trunk_rows_packed']} / {r['trunk_rows_flat']} | "
              f"{r['head_rows_packed']} / {r['head_rows_flat']} | " + " | ".join(f"{t[k]:.2f} ms" if k in t else "-" for k in ("packed", "static", "flat"))
              + f" | {ratio} |")


if __name__ == "__main__":
    main()
