"""CTC prefix beam search on the MI355X (fk_ctc_beam_search, csrc/ctc.hip) against the float64 restatement tests/ctc_beam_ref.py, on the
cases of tests/ctc_beam_cases.py.

ids and lengths must equal the restatement's exactly, for all nbest hypotheses: every case carries a margin of 16 * e32 between the
totals a selection separates (e32: what float32 arithmetic costs the restatement itself on that sample), and exact ties follow the
fixed order of the semantics.  Scores get max(4 * e32, 8 * 2^-24 * max(1, |score|)).  Both errors are printed (profiles/ctc_beam.md
records them)."""

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from tests import ctc_beam_cases as BC
from tests import ctc_cases as CC
from tests import ctc_ref as R

pytestmark = pytest.mark.gpu

KEYS = ["x", "g", "s", "m", "v", "v_bf16", "t", "l", "r"]
FLOOR = 8.0 * 2.0 ** -24


def on_gpu(case, dtype=torch.float32):
    """the case's logits on the device with the case's row stride (NaN in the padding), its input_lengths"""
    x = case["logits"]
    B, T, C = x.shape
    store = torch.full((B, T, case["ld"]), float("nan"), dtype=dtype, device="cuda")
    store[:, :, :C] = x.to(dtype).cuda()
    return store[:, :, :C], case["input_lengths"].cuda()


def run(case, dtype=torch.float32, f=K.ctc_beam_search):
    lg, il = on_gpu(case, dtype)
    return f(lg, il, blank=case["blank"], beam_width=case["W"], topk=case["K"], nbest=case["nbest"], pad=BC.PAD)


def check(case, got, label):
    """ids and lengths exact, absent slots empty, every score within its tolerance"""
    ref = case["ref"]
    ids, lengths, scores = (t.cpu().numpy() for t in got)
    assert ids.dtype == np.int64 and lengths.dtype == np.int64 and scores.dtype == np.float32
    assert np.array_equal(lengths, ref["lengths"]), (label, lengths, ref["lengths"])
    assert np.array_equal(ids, ref["ids"]), label
    have = np.isfinite(ref["scores"])
    assert np.all(np.isneginf(scores[~have])) and np.all(lengths[~have] == 0) and np.all(ids[~have] == BC.PAD)
    err = np.abs(scores[have].astype(np.float64) - ref["scores"][have])
    tol = np.maximum(4.0 * case["e32"][:, None], FLOOR * np.maximum(1.0, np.abs(ref["scores"])))[have]
    print(f"ctc beam {label:14s}: |restatement fp32 - f64| {case['e32'].max():.3e}  |kernel - f64| {err.max():.3e}  largest error / tolerance "
          f"{(err / tol).max():.2f};  max |score| {np.abs(ref['scores'][have]).max():.1f}")
    assert np.all(err <= tol), (label, err.max(), (err / tol).max())


@pytest.mark.parametrize("key", KEYS)
def test_parity_with_float64(key):
    case = BC.make(key)
    got = run(case)
    check(case, got, key)
    again = run(case)                                     # the same bits every run
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    if key == "v_bf16":                                   # the same logits as bf16 tensors, as a bf16 model gives them
        check(case, run(case, torch.bfloat16), key + " bf16")
        check(case, run(case, torch.bfloat16, E.ctc_beam_decode), key + " engine")


def test_engine_and_defaults():
    for key in ("s", "m"):
        check(BC.make(key), run(BC.make(key), f=E.ctc_beam_decode), key + " engine")
    case = BC.make("s")
    lg, il = on_gpu(case)
    B, T, C = lg.shape
    # without input_lengths every sample has T frames; nbest = 1 and the default topk = min(32, C - 1)
    ref, e32, margin = BC.measure(case["logits"].numpy(), np.full(B, T), case["blank"], case["W"], min(32, C - 1), 1)
    assert np.all(margin >= BC.MARGIN * e32)
    got = E.ctc_beam_decode(lg, blank=case["blank"], beam_width=case["W"])
    assert got[0].shape == (B, 1, T)
    check(dict(ref=ref, e32=e32), got, "s defaults")
    # lengths outside [0, T] are clamped on the device
    wild = il.clone()
    wild[0], wild[-1] = lg.shape[1] + 7, -3
    ids, lengths, scores = E.ctc_beam_decode(lg, wild, blank=case["blank"], beam_width=case["W"], topk=case["K"])
    assert int(lengths[-1, 0]) == 0 and float(scores[-1, 0]) == 0.0 and np.array_equal(ids[0, 0].cpu().numpy(), case["ref"]["ids"][0, 0])


def test_unpruned_scores_are_the_loss():
    """case x: nothing is pruned, so a score is the labelling's log-probability, which the lattice kernel computes another way"""
    case = BC.make("x")
    lg, il = on_gpu(case)
    ids, lengths, scores = run(case)
    x = case["logits"]
    for h in range(case["nbest"]):
        have = torch.isfinite(scores[:, h])
        if not bool(have.any()):
            continue
        st = K.ctc_loss_fwd(lg, ids[:, h].contiguous(), il, lengths[:, h].contiguous(), case["blank"], "none", False, want_grad=False)
        tg = dict(logits=x, targets=ids[:, h].cpu(), input_lengths=case["input_lengths"], target_lengths=lengths[:, h].cpu(), blank=case["blank"])
        ref = R.ctc(x.numpy(), tg["targets"].numpy(), tg["input_lengths"].numpy(), tg["target_lengths"].numpy(), blank=case["blank"])
        nll32, _ = CC.torch_ctc(tg, torch.float32, "none", False)
        hv = have.cpu().numpy()
        err32 = float(np.abs(nll32.numpy().astype(np.float64) - ref["nll"])[hv].max())
        tol = max(4.0 * err32, FLOOR * max(1.0, float(np.abs(ref["nll"][hv]).max())))
        diff = (scores[:, h] + st.nll)[have].abs().max().item()
        print(f"ctc beam x hypothesis {h}: |score + nll| {diff:.3e} (tol {tol:.3e})")
        assert diff <= tol, (h, diff, tol)


def test_no_host_synchronisation():
    """the call inside a stream capture (which raises on anything that waits for the host); the replay gives the eager bits"""
    case = BC.make("s")
    lg, il = on_gpu(case)

    def step():
        return E.ctc_beam_decode(lg, il, blank=case["blank"], beam_width=case["W"], topk=case["K"], nbest=case["nbest"])

    eager = step()
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


def test_model_decode(fp32_mode):
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainFormerCTC
    enc = bf.MAEConfig(window_size=200, n_electrodes=64, patch_size=25, dim=128, n_layers=2, head_dim=32, hidden_dim=512, n_heads=4, n_kv_heads=4)
    cfg = bf.Config(encoder=enc, n_output_tokens=8, output_dim=6, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4, n_kv_heads=4)
    torch.manual_seed(3)
    m = BrainFormerCTC(cfg).cuda()
    with torch.no_grad():                                 # a head that does not start at zero, so that the frames differ
        m.perceiver["to_words"].weight.normal_(0.0, 0.5)
    x = torch.randn(2, 200, 64, device="cuda")
    with torch.no_grad():
        logits = m.features(x)
    W, Kc, nbest = 4, 3, 4
    ref, e32, margin = BC.measure(logits.float().cpu().numpy(), np.array([8, 8]), m.blank, W, Kc, nbest)
    assert np.all(np.isfinite(e32)) and np.all(margin >= BC.MARGIN * e32), (e32, margin)
    case = dict(ref=ref, e32=e32)
    out = m.decode(x, beam_width=W, topk=Kc, nbest=nbest)
    assert len(out) == 3 and out[0].shape == (2, nbest, 8)
    check(case, out, "model")
    best = m.decode(x, beam_width=W, topk=Kc)
    assert len(best) == 2 and torch.equal(best[0], out[0][:, 0]) and torch.equal(best[1], out[1][:, 0])
    # without a width: today's greedy result and return type, bit for bit
    ids, lens = m.decode(x)
    want_ids, want_lens = E.ctc_greedy_decode(logits, blank=m.blank, pad=-100)
    assert torch.equal(ids, want_ids) and torch.equal(lens, want_lens)
