"""Isolated timing of the edit-distance family (csrc/editdist.hip) at the README's two CTC shapes, each beside the thing it stands next to in
a decoder or a training step, in the same interleaved rounds of one process (median of the rounds, every case warmed up first):

  error_rate      engine.error_rate on the best hypotheses, beside utils.metrics.token_error_rate on the host (copy back + Python loops)
  mbr_rerank      engine.mbr_rerank (pairwise distances + ranking, two launches) beside engine.ctc_beam_decode on the same logits, which
                  produced the list; and the host double loop (utils.metrics.edit_distance over all pairs) on two sentences, scaled to B
  ctc_mwer_loss   forward + backward beside engine.ctc_loss forward + backward on the same logits (the list is passed in: the search is the
                  line above)

Usage: python tools/wer_bench.py [rounds] [reps]
Shapes: B = 32 x (32 frames, 50258 classes, 25 labels) at beam width 5 / nbest 5, and B = 32 x (768 frames, 41 classes, 120 labels) at beam
width 32 (nbest 32 for the re-ranking, 8 for the loss: the expansion holds nbest copies of the logits and of their gradient).
No parent commit has this path, so the numbers carry no threshold; profiles/edit_distance.md records them."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from frankenstein_amd import engine as E
from frankenstein_amd.utils import metrics

#          B,  T,   C,     labels, beam width, topk, nbest of the list, nbest of the loss
SHAPES = [(32, 32,  50258, 25,     5,          20,   5,                 5),
          (32, 768, 41,    120,    32,         32,   32,                8)]
argv = sys.argv[1:]
rounds = int(argv[0]) if len(argv) > 0 else 7
reps = int(argv[1]) if len(argv) > 1 else 10
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


for B, T, C, L, W, Kc, n_list, n_loss in SHAPES:
    blank = C - 1
    logits = 2.0 * torch.randn(B, T, C, device=dev, generator=g)
    logits[:, :, blank] += 3.0
    targets = torch.randint(0, C - 1, (B, L), device=dev, generator=g)
    ids, lengths, scores = E.ctc_beam_decode(logits, None, blank, W, Kc, n_list)
    hyps = (ids[:, :n_loss].contiguous(), lengths[:, :n_loss].contiguous(), scores[:, :n_loss].contiguous())
    best, best_len = ids[:, 0].contiguous(), lengths[:, 0].contiguous()
    leaf = logits.clone().requires_grad_(True)

    def mwer():
        leaf.grad = None
        E.ctc_mwer_loss(leaf, targets, blank=blank, hyps=hyps).backward()

    def ctc():
        leaf.grad = None
        E.ctc_loss(leaf, targets, blank=blank, zero_infinity=True).backward()

    cases = {"error_rate": lambda: E.error_rate(targets, best, hypothesis_lengths=best_len),
             "mbr_rerank": lambda: E.mbr_rerank(ids, lengths, scores),
             "beam search": lambda: E.ctc_beam_decode(logits, None, blank, W, Kc, n_list),
             "mwer fwd+bwd": mwer, "ctc fwd+bwd": ctc}
    for f in cases.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for k, f in cases.items():
            times[k].append(timed(f))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}

    # the host's way: copy back, Python loops
    t0 = time.perf_counter()
    refs, hyp_rows = targets.tolist(), [r[:int(l)] for r, l in zip(best.tolist(), best_len.tolist())]
    host_rate = metrics.token_error_rate(refs, hyp_rows)
    host_er = time.perf_counter() - t0
    rate = float(E.error_rate(targets, best, hypothesis_lengths=best_len)[0])
    n_host = min(B, 2)                                    # the host walks sentence after sentence: two are timed, B are charged
    rows = [[r[:int(l)] for r, l in zip(ids[b].tolist(), lengths[b].tolist())] for b in range(n_host)]
    t0 = time.perf_counter()
    host_d = [[[metrics.edit_distance(x, y) for y in s] for x in s] for s in rows]
    host_pw = (time.perf_counter() - t0) / n_host * B
    r = E.mbr_rerank(ids, lengths, scores)
    fin = torch.isfinite(scores[:n_host])
    same = all(int(r.dist[b, i, j]) == host_d[b][i][j] for b in range(n_host) for i in range(n_list) for j in range(n_list) if fin[b, i] and fin[b, j])
    moved = int((r.order[:, 0] != 0).sum())
    print(f"(B, T, C) = ({B}, {T}, {C})  W {W} K {Kc} list {n_list} (loss: {n_loss}), targets {targets.shape[1]} labels, hypotheses up to "
          f"{int(lengths.max())} tokens:\n    " + "  ".join(f"{k} {t:9.1f} us" for k, t in med.items())
          + "\n    rounds min .. max: " + "  ".join(f"{k} {lo:.1f} .. {hi:.1f}" for k, (lo, hi) in spread.items())
          + f"\n    mbr / beam search {med['mbr_rerank'] / med['beam search']:.3f}   mwer / ctc {med['mwer fwd+bwd'] / med['ctc fwd+bwd']:.2f}"
          + f"\n    host: token_error_rate (copy back + loops) {host_er * 1e6:9.1f} us, rate {host_rate:.6f} (device {rate:.6f});  all pairs of a list "
          + f"{host_pw * 1e3:9.1f} ms ({n_host} sentences timed, scaled to {B}); device distances equal the host's: {same};  MBR moves the best "
          + f"hypothesis in {moved} of {B}", flush=True)
