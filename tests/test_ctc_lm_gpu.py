"""CTC prefix beam search with n-gram shallow fusion on the MI355X (fk_ctc_beam_search_lm, csrc/ctc.hip) against the float64 restatement
tests/ctc_lm_ref.py, on the cases of tests/ctc_lm_cases.py.

ids and lengths must equal the restatement's exactly, for all nbest hypotheses: every case carries a margin of 16 * e32 between the keys
a selection separates (e32: what float32 arithmetic costs the restatement itself on that sample), and exact ties follow the fixed order
of the semantics.  am, lm and total each get max(4 * e32, 8 * 2^-24 * max(1, |value|)), the rule of tests/test_ctc_beam_gpu.py.  The errors
are printed (profiles/ctc_lm_fusion.md records them).  No test feeds a malformed table: the bounds of the look-up are read in the code."""

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from tests import ctc_lm_cases as LC

pytestmark = pytest.mark.gpu

KEYS = ["x", "s", "b", "m", "v", "v_bf16", "t", "l", "r", "p", "e", "e_noeos"]
FLOOR = 8.0 * 2.0 ** -24


def on_gpu(case, dtype=torch.float32):
    """the case's logits on the device with the case's row stride (NaN in the padding), its input_lengths"""
    x = case["logits"]
    B, T, C = x.shape
    store = torch.full((B, T, case["ld"]), float("nan"), dtype=dtype, device="cuda")
    store[:, :, :C] = x.to(dtype).cuda()
    return store[:, :, :C], case["input_lengths"].cuda()


def run(case, dtype=torch.float32, f=K.ctc_beam_search_lm):
    lg, il = on_gpu(case, dtype)
    return f(lg, case["lm"], il, blank=case["blank"], beam_width=case["W"], topk=case["K"], nbest=case["nbest"], lm_weight=case["lm_weight"],
             length_bonus=case["length_bonus"], use_eos=case["use_eos"], pad=LC.PAD)


def check(case, got, label):
    """ids and lengths exact, absent slots empty, am, lm and total within their tolerance"""
    ref = case["ref"]
    ids, lengths, am, lm, total = (t.cpu().numpy() for t in got)
    assert ids.dtype == np.int64 and lengths.dtype == np.int64 and am.dtype == lm.dtype == total.dtype == np.float32
    assert np.array_equal(lengths, ref["lengths"]), (label, lengths, ref["lengths"])
    assert np.array_equal(ids, ref["ids"]), label
    have = np.isfinite(ref["total"])
    assert np.all(lengths[~have] == 0) and np.all(ids[~have] == LC.PAD)
    worst = []
    for name, val in (("am", am), ("lm", lm), ("total", total)):
        assert np.all(np.isneginf(val[~have])), (label, name)
        err = np.abs(val[have].astype(np.float64) - ref[name][have])
        tol = np.maximum(4.0 * case["e32"][:, None], FLOOR * np.maximum(1.0, np.abs(ref[name])))[have]
        worst.append((name, err.max(), (err / tol).max()))
    print(f"ctc lm {label:14s}: |restatement fp32 - f64| {case['e32'].max():.3e}  |kernel - f64| " +
          "  ".join(f"{n} {e:.3e} ({r:.2f} of its tolerance)" for n, e, r in worst) + f";  max |total| {np.abs(ref['total'][have]).max():.1f}")
    for name, e, r in worst:
        assert r <= 1.0, (label, name, e, r)


@pytest.mark.parametrize("key", KEYS)
def test_parity_with_float64(key):
    case = LC.make(key)
    got = run(case)
    check(case, got, key)
    again = run(case)                                     # the same bits every run
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    if key == "v_bf16":                                   # the same logits as bf16 tensors, through the engine
        check(case, run(case, torch.bfloat16), key + " bf16")
        check(case, run(case, torch.bfloat16, E.ctc_beam_decode_lm), key + " engine")


@pytest.mark.parametrize("key", ["s", "m", "t"])
def test_zero_weight_is_the_plain_search(key):
    """lm_weight = 0, length_bonus = 0, no end of sentence: ids, lengths and am are the plain search's bits"""
    case = LC.make(key)
    lg, il = on_gpu(case)
    kw = dict(blank=case["blank"], beam_width=case["W"], topk=case["K"], nbest=case["nbest"], pad=LC.PAD)
    ids, lengths, am, lm, total = E.ctc_beam_decode_lm(lg, case["lm"], il, lm_weight=0.0, length_bonus=0.0, use_eos=False, **kw)
    want = E.ctc_beam_decode(lg, il, **kw)
    assert torch.equal(ids, want[0]) and torch.equal(lengths, want[1]) and torch.equal(am, want[2]) and torch.equal(total, want[2])
    have = torch.isfinite(am)
    assert bool(torch.isfinite(lm[have]).all()) and bool((lm[have] <= 0).all()) and bool(torch.isneginf(lm[~have]).all())


def test_no_host_synchronisation():
    """the call inside a stream capture (which raises on anything that waits for the host); the replay gives the eager bits"""
    case = LC.make("s")
    lg, il = on_gpu(case)

    def step():
        return E.ctc_beam_decode_lm(lg, case["lm"], il, blank=case["blank"], beam_width=case["W"], topk=case["K"], nbest=case["nbest"],
                                    lm_weight=case["lm_weight"], length_bonus=case["length_bonus"])

    eager = step()                                        # (the first call copies the model's tables to the device)
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
    check(case, out, "s graph")


# ---- model ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def small_model():
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainFormerCTC
    enc = bf.MAEConfig(window_size=200, n_electrodes=64, patch_size=25, dim=128, n_layers=2, head_dim=32, hidden_dim=512, n_heads=4, n_kv_heads=4)
    cfg = bf.Config(encoder=enc, n_output_tokens=8, output_dim=6, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4, n_kv_heads=4)
    torch.manual_seed(3)
    m = BrainFormerCTC(cfg).cuda()
    with torch.no_grad():                                 # a head that does not start at zero, so that the frames differ
        m.perceiver["to_words"].weight.normal_(0.0, 0.5)
    return m, torch.randn(2, 200, 64, device="cuda")


def test_model_decode(fp32_mode):
    from frankenstein_amd.utils.ngram import NGramLM, zipf_sequences
    m, x = small_model()
    lm = NGramLM.from_corpus(zipf_sequences(40, 6, m.blank, (2, 8), 5), 3, 6)
    with torch.no_grad():
        logits = m.features(x)
    W, Kc, nbest, lw, bonus = 4, 3, 4, 0.8, 0.5
    ref, e32, margin = LC.measure(logits.float().cpu().numpy(), np.array([8, 8]), lm, m.blank, W, Kc, nbest, lw, bonus, True)
    assert np.all(np.isfinite(e32)) and np.all(margin >= LC.MARGIN * e32), (e32, margin)
    case = dict(ref=ref, e32=e32)
    got = E.ctc_beam_decode_lm(logits, lm, blank=m.blank, beam_width=W, topk=Kc, nbest=nbest, lm_weight=lw, length_bonus=bonus)
    check(case, got, "model")
    out = m.decode(x, beam_width=W, topk=Kc, nbest=nbest, ngram=lm, ngram_weight=lw, ngram_bonus=bonus)
    assert len(out) == 3 and out[0].shape == (2, nbest, 8)
    assert torch.equal(out[0], got[0]) and torch.equal(out[1], got[1]) and torch.equal(out[2], got[4])    # the scores are the totals
    best = m.decode(x, beam_width=W, topk=Kc, ngram=lm, ngram_weight=lw, ngram_bonus=bonus)
    assert len(best) == 2 and torch.equal(best[0], out[0][:, 0]) and torch.equal(best[1], out[1][:, 0])
    off = m.decode(x, beam_width=W, topk=Kc, nbest=nbest, ngram=lm, ngram_weight=lw, ngram_bonus=bonus, ngram_eos=False)
    want = E.ctc_beam_decode_lm(logits, lm, blank=m.blank, beam_width=W, topk=Kc, nbest=nbest, lm_weight=lw, length_bonus=bonus, use_eos=False)
    assert torch.equal(off[0], want[0]) and torch.equal(off[2], want[4])
    # without ngram: today's results, bit for bit
    plain = m.decode(x, beam_width=W, topk=Kc, nbest=nbest)
    want = E.ctc_beam_decode(logits, blank=m.blank, beam_width=W, topk=Kc, nbest=nbest, pad=-100)
    assert all(torch.equal(a, b) for a, b in zip(plain, want))
    with pytest.raises(ValueError, match="beam_width"):
        m.decode(x, ngram=lm)


def test_model_decode_with_both_language_models(fp32_mode):
    """ngram= and lm= together: the fused search fills the whole beam, the GPT rescores it on the pure CTC score"""
    from frankenstein_amd.models.gpt2_model import GPT, GPTConfig
    from frankenstein_amd.utils.ngram import NGramLM, zipf_sequences
    m, x = small_model()
    lm = NGramLM.from_corpus(zipf_sequences(40, 6, m.blank, (2, 8), 5), 3, 6)
    from tests import rescore_cases as RC
    V = 307                                               # the test model of tests/rescore_cases.py, as tests/test_rescore_gpu.py builds it
    cfg = RC.gpt_cfg(V)
    gpt = GPT(GPTConfig(block_size=cfg.block_size, vocab_size=V, n_layer=cfg.n_layer, n_head=cfg.n_head, n_embd=cfg.n_embd, bias=True)).cuda().eval()
    own = gpt.state_dict()
    with torch.no_grad():
        for k, v in RC.state_dict(V).items():
            own[k].copy_(v)
    E.bump_weight_epoch()
    W, Kc, nbest = 4, 3, 2
    kw = dict(lm_weight=0.7, length_bonus=0.2, eos_token_id=V - 1, bos_token_id=V - 1)
    out = m.decode(x, beam_width=W, topk=Kc, nbest=nbest, ngram=lm, ngram_weight=0.8, ngram_bonus=0.5, lm=gpt, **kw)
    with torch.no_grad():
        logits = m.features(x)
    ids, lengths, am, _, _ = E.ctc_beam_decode_lm(logits, lm, blank=m.blank, beam_width=W, topk=Kc, nbest=W, lm_weight=0.8, length_bonus=0.5)
    r_ids, r_lengths, _, _, r_total, _, _ = gpt.rescore_nbest(ids, lengths, am, **kw)
    assert len(out) == 3 and out[0].shape == (2, nbest, 8)
    assert torch.equal(out[0], r_ids[:, :nbest]) and torch.equal(out[1], r_lengths[:, :nbest]) and torch.equal(out[2], r_total[:, :nbest])
