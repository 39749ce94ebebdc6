"""Isolated timing of the CTC loss, forward + backward (csrc/ctc.hip), and beside it torch.nn.functional.ctc_loss on the same GPU and the
same inputs (log_softmax + ctc_loss + autograd backward: what a user would otherwise call).  Interleaved rounds in one process, median.
Usage: python tools/ctc_bench.py [rounds] [reps]   -> one line per shape (B, T, C, L): ours fwd, ours bwd, ours fwd + bwd, torch fwd + bwd, us.
No parent commit has this path: torch's number is the only yardstick."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from frankenstein_amd import kernels as K

SHAPES = [(32, 32, 50258, 25), (32, 128, 41, 40), (32, 768, 41, 120)]
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
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


for B, T, C, L in SHAPES:
    blank = C - 1
    logits = 3.0 * torch.randn(B, T, C, device=dev, generator=g)
    targets = torch.randint(0, C - 1, (B, L), device=dev, generator=g)
    il = torch.full((B,), T, dtype=torch.int64, device=dev)
    tl = torch.full((B,), L, dtype=torch.int64, device=dev)
    gout = torch.ones(1, device=dev)
    dl = torch.empty_like(logits)
    leaf = logits.clone().requires_grad_(True)
    state = {}

    def ours_fwd():
        state["st"] = K.ctc_loss_fwd(logits, targets, il, tl, blank, "mean", True)

    def ours_bwd():
        K.ctc_loss_bwd(logits, state["st"], gout, dl)

    def ours():
        ours_fwd()
        ours_bwd()

    def theirs():
        leaf.grad = None
        F.ctc_loss(F.log_softmax(leaf, -1).transpose(0, 1), targets, il, tl, blank=blank, reduction="mean", zero_infinity=True).backward()

    cases = {"ours fwd": ours_fwd, "ours bwd": ours_bwd, "ours fwd+bwd": ours, "torch fwd+bwd": theirs}
    for f in cases.values():
        f()
    torch.cuda.synchronize()
    err = float((dl - leaf.grad).abs().max())
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for k, f in cases.items():
            times[k].append(timed(f))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(f"(B, T, C, L) = ({B}, {T}, {C}, {L})  route {K.CTC_ROUTE_NAMES[K.ctc_route(L)]:8s} " + "  ".join(f"{k} {t:8.1f} us" for k, t in med.items())
          + f"  ours / torch {med['ours fwd+bwd'] / med['torch fwd+bwd']:.2f}  max |dlogits - torch| {err:.2e}", flush=True)
