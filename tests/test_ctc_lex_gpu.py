"""Lexicon-constrained CTC prefix beam search on the MI355X (fk_ctc_beam_search_lex, csrc/ctc.hip) against the float64 restatement
tests/ctc_lex_ref.py, on the cases of tests/ctc_lex_cases.py.

words, word_lengths, ids, lengths and complete must equal the restatement's exactly, for all nbest hypotheses: every case carries a
margin of 16 * e32 between the keys a selection separates and between the homophones a word end chooses among (e32: what float32
arithmetic costs the restatement itself on that sample), and exact ties follow the fixed order of the semantics.  am, lm and total each get
max(4 * e32, 8 * 2^-24 * max(1, |value|)), the rule of tests/test_ctc_lm_gpu.py.  The errors are printed (profiles/ctc_lexicon.md records
them).  No test feeds a malformed table: the bounds of the look-ups are read in the code and stated in the header."""

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from tests import ctc_lex_cases as XC
from tests import ctc_lex_ref as XR
from tests import edit_ref as ER
from tests.ctc_lm_cases import MARGIN, PAD

pytestmark = pytest.mark.gpu

FLOOR = 8.0 * 2.0 ** -24
NAMES = ("words", "word_lengths", "ids", "lengths", "am", "lm", "total", "complete")


def on_gpu(case, dtype=torch.float32):
    """the case's logits on the device with the case's row stride (NaN in the padding), its input_lengths"""
    x = case["logits"]
    B, T, C = x.shape
    store = torch.full((B, T, case["ld"]), float("nan"), dtype=dtype, device="cuda")
    store[:, :, :C] = x.to(dtype).cuda()
    return store[:, :, :C], case["input_lengths"].cuda()


def run(case, dtype=torch.float32, f=K.ctc_beam_search_lex):
    lg, il = on_gpu(case, dtype)
    return f(lg, case["lexicon"], case["lm"], sep=case["sep"], input_lengths=il, blank=case["blank"], beam_width=case["W"], topk=case["K"],
             nbest=case["nbest"], lm_weight=case["lm_weight"], word_bonus=case["word_bonus"], use_eos=case["use_eos"], pad=PAD)


def check(case, got, label):
    """words, word_lengths, ids, lengths and complete exact, absent slots empty, am, lm and total within their tolerance"""
    ref = case["ref"]
    g = {n: t.cpu().numpy() for n, t in zip(NAMES, got)}
    assert all(g[n].dtype == np.int64 for n in NAMES[:4]) and all(g[n].dtype == np.float32 for n in NAMES[4:7]) and g["complete"].dtype == np.uint8
    for n in ("lengths", "ids", "word_lengths", "words", "complete"):
        assert g[n].shape == ref[n].shape and np.array_equal(g[n], ref[n]), (label, n, g[n], ref[n])
    have = np.isfinite(ref["total"])
    assert np.all(g["lengths"][~have] == 0) and np.all(g["ids"][~have] == PAD) and np.all(g["words"][~have] == PAD) and np.all(g["complete"][~have] == 0)
    worst = []
    for name in ("am", "lm", "total"):
        val = g[name]
        assert np.all(np.isneginf(val[~have])), (label, name)
        err = np.abs(val[have].astype(np.float64) - ref[name][have])
        tol = np.maximum(4.0 * case["e32"][:, None], FLOOR * np.maximum(1.0, np.abs(ref[name])))[have]
        worst.append((name, err.max(), (err / tol).max()))
    print(f"ctc lex {label:14s}: |restatement fp32 - f64| {case['e32'].max():.3e}  |kernel - f64| " +
          "  ".join(f"{n} {e:.3e} ({r:.2f} of its tolerance)" for n, e, r in worst) + f";  max |total| {np.abs(ref['total'][have]).max():.1f}")
    for name, e, r in worst:
        assert r <= 1.0, (label, name, e, r)


@pytest.mark.parametrize("key", XC.KEYS)
def test_parity_with_float64(key):
    case = XC.make(key)
    got = run(case)
    check(case, got, key)
    again = run(case)                                     # the same bits every run
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    if key == "p_bf16":                                   # the same logits as bf16 tensors, through the engine
        check(case, run(case, torch.bfloat16), key + " bf16")
        check(case, tuple(run(case, torch.bfloat16, E.ctc_beam_decode_lexicon)), key + " engine")


def test_planted_words_come_back():
    """logits peaked on the pronunciation of a planted word sequence: the decoded words are the planted ones (no restatement involved)"""
    pl = XC.planted()
    r = E.ctc_beam_decode_lexicon(pl["logits"].cuda(), pl["lexicon"], pl["lm"], sep=pl["sep"], input_lengths=pl["input_lengths"].cuda(),
                                  blank=pl["blank"], beam_width=8, topk=8, nbest=2, lm_weight=0.5)
    for b, ws in enumerate(pl["words"]):
        assert r.words[b, 0, :len(ws)].tolist() == ws and int(r.word_lengths[b, 0]) == len(ws) and int(r.complete[b, 0]) == 1
        assert bool((r.words[b, 0, len(ws):] == -100).all())
        assert r.ids[b, 0, :int(r.lengths[b, 0])].tolist() == pl["lexicon"].pronounce(ws, pl["sep"])
    assert pl["lexicon"].text(r.words[:, 0], r.word_lengths[:, 0]) == [" ".join(f"w{w}" for w in ws) for ws in pl["words"]]


def test_am_is_the_plain_search_mass():
    """lm=None, word_bonus = 0, no end of sentence, and a lexicon that admits whatever the plain search can form (every sequence of up to T
    non-sep classes is a word; sep is never a candidate: its logit is the lowest and K = C - 2): the recursion is the plain search's, so
    ids, lengths and am are fk_ctc_beam_search's bits for every hypothesis, each non-empty labelling is one closed word, all are complete"""
    import itertools
    from frankenstein_amd.utils.lexicon import Lexicon
    B, T, C, blank, sep, W = 3, 6, 5, 0, 1, 6
    phones = [c for c in range(C) if c not in (blank, sep)]
    free = Lexicon(("".join(map(str, p)), p) for n in range(1, T + 1) for p in itertools.product(phones, repeat=n))
    g = torch.Generator().manual_seed(77)
    x = 2.0 * torch.randn((B, T, C), generator=g)
    x[:, :, blank] += 3.0
    x[:, :, sep] = -30.0
    lg, il = x.cuda(), torch.tensor([T, T - 2, 1]).cuda()
    r = E.ctc_beam_decode_lexicon(lg, free, None, sep=sep, input_lengths=il, blank=blank, beam_width=W, topk=C - 2, nbest=W, lm_weight=0.0,
                                  word_bonus=0.0, use_eos=False)
    ids, lengths, scores = E.ctc_beam_decode(lg, il, blank=blank, beam_width=W, topk=C - 2, nbest=W)
    assert torch.equal(r.ids, ids) and torch.equal(r.lengths, lengths) and torch.equal(r.am, scores) and torch.equal(r.total, scores)
    have = torch.isfinite(scores)
    assert int(have.sum()) > B and torch.equal(r.complete.bool(), have) and torch.equal(r.word_lengths, ((lengths > 0) & have).long())
    assert bool((r.lm[have] == 0).all())
    for b in range(B):
        for h in range(W):
            if int(r.word_lengths[b, h]):
                assert free.words[int(r.words[b, h, 0])] == "".join(map(str, ids[b, h, :int(lengths[b, h])].tolist()))


def test_no_host_synchronisation():
    """the call inside a stream capture (which raises on anything that waits for the host); the replay gives the eager bits"""
    case = XC.make("h")
    lg, il = on_gpu(case)

    def step():
        return E.ctc_beam_decode_lexicon(lg, case["lexicon"], case["lm"], sep=case["sep"], input_lengths=il, blank=case["blank"], beam_width=case["W"],
                                         topk=case["K"], nbest=case["nbest"], lm_weight=case["lm_weight"], word_bonus=case["word_bonus"])

    eager = step()                                        # (the first call copies the tables to the device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    check(case, tuple(out), "h graph")


def _lists(ref, b, n):
    """the restatement's word lists of sample b, padded to n hypotheses -> (rows, lengths, scores)"""
    hyps = ref["hyps"][b][:n]
    L = ref["words"].shape[2]
    rows = [list(h[4]) + [PAD] * (L - len(h[4])) for h in hyps] + [[PAD] * L] * (n - len(hyps))
    return rows, [len(h[4]) for h in hyps] + [0] * (n - len(hyps)), [h[3] for h in hyps] + [-np.inf] * (n - len(hyps))


@pytest.mark.parametrize("key", ["h", "c"])
def test_composes_with_error_rate_oracle_and_mbr(key):
    """engine.error_rate, nbest_oracle and mbr_rerank on `words` equal tests/edit_ref.py on the restatement's lists"""
    case = XC.make(key)
    ref = case["ref"]
    lg, il = on_gpu(case)
    r = E.ctc_beam_decode_lexicon(lg, case["lexicon"], case["lm"], sep=case["sep"], input_lengths=il, blank=case["blank"],
                                  beam_width=case["W"], topk=case["K"], nbest=case["nbest"], lm_weight=case["lm_weight"], word_bonus=case["word_bonus"])
    B, n = ref["words"].shape[:2]
    targets = torch.full((B, 4), -100, dtype=torch.int64)
    want_err, want_best = [], []
    for b in range(B):
        t = [0, 3, 1][:2 + b]
        targets[b, :len(t)] = torch.tensor(t)
        rows, lens, scores = _lists(ref, b, n)
        d = [ER.distance(t, rows[h][:lens[h]]) if np.isfinite(scores[h]) else 2 ** 31 - 1 for h in range(n)]
        want_err.append(d[0])
        want_best.append((min(d), d.index(min(d))))
    rate, errors, ref_lengths = E.error_rate(targets.cuda(), r.words[:, 0], hypothesis_lengths=r.word_lengths[:, 0])
    assert errors.tolist() == want_err and abs(float(rate) - sum(want_err) / float(ref_lengths.sum())) < 1e-6
    best, index = E.nbest_oracle(r.words, r.word_lengths, r.total, targets.cuda())
    assert list(zip(best.tolist(), index.tolist())) == want_best
    m = E.mbr_rerank(r.words, r.word_lengths, r.total, scale=1.0)
    for b in range(B):
        rows, lens, scores = _lists(ref, b, n)
        dist = ER.pairwise(rows, lens, scores)
        assert np.array_equal(m.dist[b].cpu().numpy(), dist), (key, b)
        risk64, order64, nv = ER.mbr(dist, scores, 1.0, np.float64)
        risk32, order32, _ = ER.mbr(dist, scores, 1.0, np.float32)
        ok = np.isfinite(np.asarray(risk64, dtype=np.float64))
        e32 = np.abs(np.asarray(risk64, dtype=np.float64)[ok] - np.asarray(risk32, dtype=np.float64)[ok]).max()
        assert list(order64) == list(order32), (key, b)
        assert ER.smallest_gap(risk64, ok) >= MARGIN * e32, (key, b)  # risks far enough apart for float32 to order them: the CPU decides
        assert m.order[b].tolist() == [int(i) for i in order64] and int(m.n_valid[b]) == nv, (key, b)


# ---- model ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def test_model_decode_words(fp32_mode):
    """BrainFormerCTC.decode_words / word_error_rate on the small model of tests/test_ctc_lm_gpu.py equal the restatement on its logits"""
    from tests.test_ctc_lm_gpu import small_model
    m, x = small_model()                                  # 6 classes, blank 5, 8 frames
    lex, lm, sep = XC.lexicon("h"), XC.model("h"), 1      # pronunciations over the classes 2, 3, 4
    prons, prefixes = XR.lexicon_dicts(lex)
    with torch.no_grad():
        logits = m.features(x)
    W, Kc, nbest, lw, bonus = 4, 4, 4, 0.8, 0.5
    ref, e32, margin = XC.measure(logits.float().cpu().numpy(), np.array([8, 8]), prons, prefixes, lm, m.blank, sep, W, Kc, nbest, lw, bonus)
    assert np.all(np.isfinite(e32)) and np.all(margin >= MARGIN * e32), (e32, margin)
    got = E.ctc_beam_decode_lexicon(logits, lex, lm, sep=sep, blank=m.blank, beam_width=W, topk=Kc, nbest=nbest, lm_weight=lw, word_bonus=bonus)
    check(dict(ref=ref, e32=e32), tuple(got), "model")
    out = m.decode_words(x, lex, sep, beam_width=W, topk=Kc, nbest=nbest, ngram=lm, ngram_weight=lw, word_bonus=bonus)
    assert len(out) == 3 and out[0].shape == (2, nbest, 4)
    assert torch.equal(out[0], got.words) and torch.equal(out[1], got.word_lengths) and torch.equal(out[2], got.total)
    best = m.decode_words(x, lex, sep, beam_width=W, topk=Kc, ngram=lm, ngram_weight=lw, word_bonus=bonus)
    assert len(best) == 2 and torch.equal(best[0], got.words[:, 0]) and torch.equal(best[1], got.word_lengths[:, 0])
    ranked = m.decode_words(x, lex, sep, beam_width=W, topk=Kc, nbest=2, ngram=lm, ngram_weight=lw, word_bonus=bonus, mbr=True)
    want = E.mbr_rerank(got.words, got.word_lengths, got.total)
    assert torch.equal(ranked[0], want.ids[:, :2]) and torch.equal(ranked[1], want.lengths[:, :2]) and torch.equal(ranked[2], -want.risk[:, :2])
    targets = torch.tensor([[0, 3, -100], [3, 1, 4]], device="cuda")
    rate, errors, ref_lengths = m.word_error_rate(x, targets, lex, sep, beam_width=W, topk=Kc, ngram=lm, ngram_weight=lw, word_bonus=bonus)
    want_err = [ER.distance([0, 3], ref["hyps"][0][0][4]), ER.distance([3, 1, 4], ref["hyps"][1][0][4])]
    assert errors.tolist() == want_err and ref_lengths.tolist() == [2, 3] and abs(float(rate) - sum(want_err) / 5.0) < 1e-6
    # decode keeps its behaviour: the plain beam search, bit for bit
    plain = m.decode(x, beam_width=W, topk=Kc, nbest=nbest)
    assert all(torch.equal(a, b) for a, b in zip(plain, E.ctc_beam_decode(logits, blank=m.blank, beam_width=W, topk=Kc, nbest=nbest, pad=-100)))
