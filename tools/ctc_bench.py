"""Isolated timing of the CTC loss, forward + backward (csrc/ctc.hip), and beside it torch.nn.functional.ctc_loss on the same GPU and the
same inputs (log_softmax + ctc_loss + autograd backward: what a user would otherwise call).  Interleaved rounds in one process, median.
Usage: python tools/ctc_bench.py [rounds] [reps]   -> one line per shape (B, T, C, L): ours fwd, ours bwd, ours fwd + bwd, torch fwd + bwd, us.
No parent commit has this path: torch's number is the only yardstick.

python tools/ctc_bench.py --beam W [rounds] [reps]: the prefix beam search (engine.ctc_beam_decode, beam width W, both launches) beside the
greedy decode on the same GPU and the same logits, and beside the float64 host restatement (tests/ctc_beam_ref.py) on the host, at the
project's vocabulary (32 frames, 50258 classes, 20 candidates) and at a phoneme head (768 frames, 41 classes, min(32, C - 1) candidates),
B = 32 each.  torch has no CTC beam search: the host restatement is the only alternative a user has.

python tools/ctc_bench.py --beam W --ngram ORDER [rounds] [reps]: also the search with n-gram shallow fusion (engine.ctc_beam_decode_lm) on
the same logits, in the same interleaved rounds: an interpolated Witten-Bell model of that order from 2000 seeded Zipf-distributed
sequences over the head's classes (utils.ngram), with its table size and max_probe, and what the fusion adds per frame.

python tools/ctc_bench.py --beam W --lexicon N_WORDS [--ngram ORDER] [rounds] [reps]: also the lexicon-constrained search
(engine.ctc_beam_decode_lexicon) in the same interleaved rounds: a seeded synthetic lexicon of N_WORDS words (utils.lexicon.zipf_lexicon,
pronunciations of 2 .. 6 classes, the separator is class C - 2 and gets + 1.5 on a copy of the logits so that words end) with a
Witten-Bell word model of order ORDER (3 without --ngram) from 2000 seeded Zipf-distributed word sequences, and the same search without
a word model: the difference between the two is what the word-LM look-ups cost, the rest over the plain search is the trie.

python tools/ctc_bench.py --align [rounds] [reps]: the forced alignment (engine.ctc_forced_align, both launches) beside the CTC loss forward
without lattice (K.ctc_loss_fwd(want_grad=False): the same row_lse launch and the same sweep with logsumexp for max) at the same shape in
the same interleaved rounds, and beside the float64 host restatement (tests/ctc_align_ref.py), at B = 32, 32 x 50258 with 25 labels and
768 x 41 with 120 labels."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K

SHAPES = [(32, 32, 50258, 25), (32, 128, 41, 40), (32, 768, 41, 120)]
BEAM_SHAPES = [(32, 32, 50258, 20), (32, 768, 41, 32)]         # B, T, C, K
argv = sys.argv[1:]
beam = int(argv.pop(argv.index("--beam") + 1)) if "--beam" in argv else None
if beam is not None:
    argv.remove("--beam")
ngram = int(argv.pop(argv.index("--ngram") + 1)) if "--ngram" in argv else None
if ngram is not None:
    argv.remove("--ngram")
lexicon = int(argv.pop(argv.index("--lexicon") + 1)) if "--lexicon" in argv else None
if lexicon is not None:
    argv.remove("--lexicon")
align = "--align" in argv
if align:
    argv.remove("--align")
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


for B, T, C, Kc in (BEAM_SHAPES if beam is not None else []):
    from tests import ctc_beam_ref as BR
    blank = C - 1
    logits = 2.0 * torch.randn(B, T, C, device=dev, generator=g)
    logits[:, :, blank] += 3.0
    cases = {"beam": lambda: E.ctc_beam_decode(logits, None, blank, beam, Kc, beam), "greedy": lambda: E.ctc_greedy_decode(logits, None, blank)}
    if ngram is not None:
        from frankenstein_amd.utils.ngram import NGramLM, zipf_sequences
        lm = NGramLM.from_corpus(zipf_sequences(2000, C, blank, (5, 20) if C > 1024 else (10, 40), 0, n_types=min(C - 1, 5000)), ngram, C)
        tab = lm.compile()
        cases["fused"] = lambda: E.ctc_beam_decode_lm(logits, lm, None, blank, beam, Kc, beam, 0.8, 0.5)
    if lexicon is not None:
        from frankenstein_amd.utils.lexicon import zipf_lexicon
        from frankenstein_amd.utils.ngram import NGramLM, zipf_sequences
        sep = C - 2
        lex = zipf_lexicon(lexicon, C, blank, sep, (2, 6), 0, 0.1)
        wlm = NGramLM.from_corpus(zipf_sequences(2000, lexicon + 1, lexicon, (5, 20), 0), ngram or 3, lexicon)
        ltab, wtab = lex.compile(), wlm.compile()
        lex_logits = logits.clone()
        lex_logits[:, :, sep] += 1.5
        cases["lex"] = lambda: E.ctc_beam_decode_lexicon(lex_logits, lex, wlm, sep, None, blank, beam, Kc, beam, 0.8, 0.5)
        cases["lex no model"] = lambda: E.ctc_beam_decode_lexicon(lex_logits, lex, None, sep, None, blank, beam, Kc, beam, 0.8, 0.5)
    for f in cases.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for k, f in cases.items():
            times[k].append(timed(f))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    ids, lengths, scores = cases["beam"]()
    g_ids, g_len = cases["greedy"]()
    differ = int(((lengths[:, 0] != g_len) | (ids[:, 0] != g_ids).any(1)).sum())
    n_host = min(B, 2)                                         # the host walks sample after sample: two are timed, B are charged
    x = logits[:n_host].cpu().numpy()
    t0 = time.perf_counter()
    ref = BR.beam_search(x, None, blank, beam, Kc, beam)
    host = (time.perf_counter() - t0) / n_host * B
    same = bool((ids[:n_host, 0].cpu().numpy() == ref["ids"][:, 0]).all())
    print(f"(B, T, C) = ({B}, {T}, {C})  W {beam} K {Kc} nbest {beam}:  " + "  ".join(f"{k} {t:9.1f} us" for k, t in med.items())
          + f"  host float64 restatement {host * 1e3:9.1f} ms ({n_host} samples timed, scaled to {B})  best hypothesis differs from greedy in {differ} of {B}"
          + f"  best ids equal the restatement's: {same}", flush=True)
    if ngram is not None:
        spread = {k: (min(v), max(v)) for k, v in times.items()}
        moved = int((cases["fused"]()[0][:, 0] != ids[:, 0]).any(1).sum())
        print(f"    order {ngram}: {tab.n_entries} n-grams in {tab.cap} entries ({tab.cap * 16 / 1024:.0f} KiB), {tab.n_states} states, max_probe {tab.max_probe};  "
              f"fused - beam {med['fused'] - med['beam']:+9.1f} us = {(med['fused'] - med['beam']) / T:+.3f} us per frame, fused / beam {med['fused'] / med['beam']:.2f};  "
              f"rounds min .. max: beam {spread['beam'][0]:.1f} .. {spread['beam'][1]:.1f} us, fused {spread['fused'][0]:.1f} .. {spread['fused'][1]:.1f} us;  "
              f"the best hypothesis moves in {moved} of {B}", flush=True)
    if lexicon is not None:
        spread = {k: (min(v), max(v)) for k, v in times.items()}
        r = cases["lex"]()
        print(f"    lexicon {lexicon} words: {ltab.n_nodes} trie nodes in {ltab.cap} entries ({ltab.cap * 16 / 1024:.0f} KiB), max_probe {ltab.max_probe}; word model order "
              f"{wlm.order}: {wtab.n_entries} n-grams, max_probe {wtab.max_probe};  lex - beam {med['lex'] - med['beam']:+9.1f} us = {(med['lex'] - med['beam']) / T:+.3f} us per frame, "
              f"lex / beam {med['lex'] / med['beam']:.2f};  of it the word-LM look-ups (lex - lex no model) {med['lex'] - med['lex no model']:+9.1f} us, the trie and the "
              f"rest (lex no model - beam) {med['lex no model'] - med['beam']:+9.1f} us;  rounds min .. max: " + ", ".join(f"{k} {a:.1f} .. {b:.1f} us" for k, (a, b) in spread.items())
              + f";  complete best hypotheses {int(r.complete[:, 0].sum())} of {B}, words in them {float(r.word_lengths[:, 0].float().mean()):.1f} on average", flush=True)

for B, T, C, L in ([SHAPES[0], SHAPES[2]] if align else []):
    from tests import ctc_align_ref as AR
    blank = C - 1
    logits = 3.0 * torch.randn(B, T, C, device=dev, generator=g)
    targets = torch.randint(0, C - 1, (B, L), device=dev, generator=g)
    il = torch.full((B,), T, dtype=torch.int64, device=dev)
    tl = torch.full((B,), L, dtype=torch.int64, device=dev)
    cases = {"align": lambda: E.ctc_forced_align(logits, targets, il, tl, blank),
             "loss fwd": lambda: K.ctc_loss_fwd(logits, targets, il, tl, blank, "mean", True, want_grad=False)}
    for f in cases.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for k, f in cases.items():
            times[k].append(timed(f))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}
    r = cases["align"]()
    n_host = min(B, 2)                                         # the host walks sample after sample: two are timed, B are charged
    t0 = time.perf_counter()
    ref = AR.viterbi(logits[:n_host].cpu().numpy(), targets[:n_host].cpu().numpy(), None, None, blank)
    host = (time.perf_counter() - t0) / n_host * B
    same = bool((r.path[:n_host].cpu().numpy() == ref["path"]).all())
    feasible = int(torch.isfinite(r.score).sum())
    print(f"(B, T, C, L) = ({B}, {T}, {C}, {L})  route {K.CTC_ROUTE_NAMES[K.ctc_route(L)]:8s} " + "  ".join(f"{k} {t:8.1f} us" for k, t in med.items())
          + f"  align / loss fwd {med['align'] / med['loss fwd']:.2f}  rounds min .. max: align {spread['align'][0]:.1f} .. {spread['align'][1]:.1f} us, "
          + f"loss fwd {spread['loss fwd'][0]:.1f} .. {spread['loss fwd'][1]:.1f} us  host float64 restatement {host * 1e3:9.1f} ms ({n_host} samples timed, "
          + f"scaled to {B})  samples with an alignment {feasible} of {B}  paths equal the restatement's: {same}", flush=True)

for B, T, C, L in (SHAPES if beam is None and not align else []):
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
