"""CPU-side checks of joint CTC / attention decoding: the numpy restatement of the prefix scorer (tests/ctc_prefix_ref.py) against
brute-force enumeration of every path and against the CTC restatement (tests/ctc_ref.py), its telescoping and floor rules, the torch
form the re-forward paths use (gpt2_model._CtcPrefixHost) against it, the argument checks of GPT.generate_beam_search and of the two
entry points (FK_EINVAL before any launch; fake pointers), and the decision margins of the cases tests/test_ctc_prefix_gpu.py runs."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import ctc_prefix_cases as CC
from tests import ctc_prefix_ref as R
from tests import ctc_ref

EINVAL = -1
P = 4096          # a fake, 16-byte aligned "device pointer": never dereferenced by a refused call
f32, f64 = np.float32, np.float64


# =============================================================================================== the rule against brute force
@pytest.mark.parametrize("T,C,blank", [(1, 3, 2), (2, 3, 0), (3, 4, 3), (4, 3, 1), (5, 3, 2), (4, 4, 0)])
def test_restatement_equals_path_enumeration(T, C, blank):
    """every prefix of up to three labels (the empty one, repeated labels, prefixes no path of T frames can spell): psi and the eos term
    against the sum over all C^T paths"""
    rng = np.random.default_rng(100 * T + 10 * C + blank)
    y = R.log_softmax_rows(rng.standard_normal((T, C)) * 2)
    labels = [c for c in range(C) if c != blank]
    worst, impossible = 0.0, 0
    for L in range(4):
        for pre in itertools.product(labels, repeat=L):
            h = R.hyp_of(y, blank, list(pre))
            for got, want in ((h.psi[0], R.brute_prefix(y, blank, pre)), (R.full(h)[0], R.brute_prefix(y, blank, pre, whole=True))):
                if np.isinf(want):
                    assert got == -np.inf, (pre, got)
                    impossible += 1
                else:
                    worst = max(worst, abs(got - want))
    print(f"T={T} C={C}: worst |restatement - enumeration| = {worst:.3g}, {impossible} impossible prefixes / labellings")
    assert worst <= 1e-13
    assert impossible > 0 or T >= 5
    if T == 1:                                             # one frame: psi of one label is its log-probability, two labels do not fit
        assert R.hyp_of(y, blank, [labels[0]]).psi[0] == y[0, labels[0]] and R.hyp_of(y, blank, [labels[0], labels[1]]).psi[0] == -np.inf


@pytest.mark.parametrize("seed", range(4))
def test_eos_term_is_the_ctc_log_probability(seed):
    rng = np.random.default_rng(seed)
    T, C, blank = int(rng.integers(6, 30)), int(rng.integers(3, 12)), 0
    logits = rng.standard_normal((1, T, C)) * 2
    n = int(rng.integers(0, 6))
    tgt = rng.integers(1, C, n)
    if n >= 2:
        tgt[1] = tgt[0]                                    # a repeated label: a blank is required between them
    y = R.log_softmax_rows(logits[0])
    h = R.hyp_of(y, blank, tgt.tolist())
    nll = ctc_ref.ctc(logits, tgt[None, :] if n else np.zeros((1, 0), np.int64), target_lengths=[n], blank=blank)["raw"][0]
    assert abs(R.full(h)[0] + nll) <= 1e-12 * max(1.0, abs(nll))
    d = R.delta(y, blank, h, [C + 5], eos=C + 5)           # the eos id need not be a class
    assert abs(d[0] - (-nll - h.psi[0])) <= 1e-12 * max(1.0, abs(nll))


def test_deltas_telescope_to_psi():
    rng = np.random.default_rng(5)
    T, C, blank = 12, 7, 6
    y = R.log_softmax_rows(rng.standard_normal((T, C)) * 2)
    seq = [3, 3, 1, 0, 0, 5]
    h, tot = R.empty(y, blank), 0.0
    for c in seq:
        tot += R.delta(y, blank, h, [c])[0]
        h = R.extend(y, blank, h, [c])
        assert abs(tot - h.psi[0]) <= 1e-12 * abs(h.psi[0])
    tot += R.delta(y, blank, h, [2], eos=2)[0]
    assert abs(tot - R.full(h)[0]) <= 1e-12 * abs(tot)


def test_every_floor_condition():
    rng = np.random.default_rng(6)
    T, C, blank = 3, 4, 3
    y = R.log_softmax_rows(rng.standard_normal((T, C)))
    h = R.hyp_of(y, blank, [1])
    floor = f64(R.FLOOR)
    assert R.delta(y, blank, h, [0])[0] != floor                                          # the control: a label that fits
    assert R.delta(y, blank, h, [blank])[0] == floor                                      # c == blank
    assert R.delta(y, blank, h, [C])[0] == floor and R.delta(y, blank, h, [-1])[0] == floor   # c >= C, c < 0
    hh = R.hyp_of(y, blank, [1, 1])                                                       # 1 _ 1 takes all three frames
    assert np.isfinite(hh.psi[0]) and R.delta(y, blank, hh, [1])[0] == floor              # psi' = -inf
    assert R.delta(y, blank, R.hyp_of(y, blank, [1, 1, 1]), [0])[0] == floor              # psi = -inf
    assert R.delta(y, blank, R.hyp_of(y, blank, [C + 1]), [0])[0] == floor                # a hypothesis that took a label outside the classes
    assert R.delta(y[:0], blank, R.empty(y[:0], blank), [0], eos=2)[0] == floor           # T_g == 0, eos included
    assert R.delta(y[:0], blank, R.empty(y[:0], blank), [2], eos=2)[0] == floor
    assert R.delta(y, blank, R.hyp_of(y, blank, [1, 1, 1]), [2], eos=2)[0] == floor       # eos behind an impossible hypothesis
    # the joint value of a floor entry is finite and exact in fp32: (1 - w) * lp + w * FLOOR
    j = R.joint(f32(-1.5), f32(R.FLOOR), 0.3, f32)
    assert np.isfinite(j) and j == f32(f32(f32(1) - f32(0.3)) * f32(-1.5)) + f32(f32(0.3) * f32(R.FLOOR))


# =============================================================================================== the torch form of the re-forward paths
@pytest.mark.parametrize("Tg,eos", [(9, 2), (5, -1), (0, 2), (1, 2)])
def test_host_scorer_equals_the_restatement(Tg, eos):
    from frankenstein_amd.models.gpt2_model import _CtcPrefixHost
    rng = np.random.default_rng(40 + Tg)
    T, C, blank, W, k, w = 9, 8, 7, 3, 6, 0.3
    logits = rng.standard_normal((T, C)).astype(f32) * 2
    y = R.log_softmax_rows(logits[:Tg], f64)
    host = _CtcPrefixHost(torch.from_numpy(logits), Tg, blank, w, None if eos < 0 else eos, W, prompt_labels=[4])
    h = R.extend(y, blank, R.empty(y, blank, W), [4] * W)
    fin = np.array([0, 1, 0])
    for step in range(4):
        top_lp = (-rng.random((W, k)) * 4).astype(f32)
        top_id = np.stack([rng.choice(np.arange(-1, C + 2), k, replace=False) for _ in range(W)])
        top_id[0, 0] = h.last[0]
        want, floor = R.score_rows([y], blank, [h], top_lp, top_id, w, eos, fin, W)
        got = host.score(torch.from_numpy(top_lp), torch.from_numpy(top_id), torch.from_numpy(fin)).numpy()
        assert np.array_equal(got[floor], R.joint(top_lp, np.full_like(top_lp, R.FLOOR), w, f32)[floor])
        assert np.array_equal(got[1], top_lp[1])                                          # the finished row
        assert np.abs(got - want)[~floor].max(initial=0.0) <= 2e-5
        parent, tok = rng.integers(0, W, W), np.array([h.last[0] if h.last[0] >= 0 else 1, int(rng.integers(0, blank)), C + 3 if step == 2 else 2])
        host.advance(torch.from_numpy(parent), torch.from_numpy(tok))
        h = R.extend(y, blank, h.take(parent), tok)
        assert np.array_equal(host.last.numpy(), h.last)
        for a, b in ((host.psi.numpy(), h.psi), (host.r_n.numpy(), h.r_n), (host.r_b.numpy(), h.r_b)):
            assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.abs(a[np.isfinite(b)] - b[np.isfinite(b)]).max(initial=0.0) <= 2e-5


# =============================================================================================== argument checks
def _tiny_gpt():
    from frankenstein_amd.models.gpt2_model import GPT, GPTConfig
    return GPT(GPTConfig(block_size=32, vocab_size=64, n_layer=1, n_head=2, n_embd=16))


def test_generate_beam_search_refuses_bad_ctc_arguments_before_anything_runs(monkeypatch):
    g = _tiny_gpt()
    monkeypatch.setattr(g, "forward", lambda *a, **k: pytest.fail("the model ran"))
    idx, pf, lg = torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 4, 16)), torch.zeros((2, 5, 66))
    call = lambda **kw: g.generate_beam_search(idx, 4, pf, topk=4, beam_width=2, **kw)
    for bad in (-0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="ctc_weight"):
            call(ctc_logits=lg, ctc_weight=bad)
    with pytest.raises(ValueError, match="needs ctc_logits"):
        call(ctc_weight=0.3)
    for shape in ((3, 5, 66), (5, 66), (2, 5, 1), (2, 0, 66), (2, 5, 66, 1)):
        with pytest.raises(ValueError, match="ctc_logits must be"):
            call(ctc_logits=torch.zeros(shape), ctc_weight=0.3)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        call(ctc_logits=lg.double(), ctc_weight=0.3)
    for blank in (-1, 66, 1.0, True):
        with pytest.raises(ValueError, match="ctc_blank"):
            call(ctc_logits=lg, ctc_weight=0.3, ctc_blank=blank)
    for lens in (torch.tensor([5]), torch.tensor([[5, 5]]), torch.tensor([5.0, 5.0])):
        with pytest.raises(ValueError, match="ctc_input_lengths"):
            call(ctc_logits=lg, ctc_weight=0.3, ctc_input_lengths=lens)
    for fp in (-1, 4, 1.0):
        with pytest.raises(ValueError, match="ctc_from_prompt"):
            call(ctc_logits=lg, ctc_weight=0.3, ctc_from_prompt=fp)
    with pytest.raises(ValueError, match="ctc_blank"):                                    # checked with weight 0 too: a typo does not hide
        call(ctc_logits=lg, ctc_weight=0.0, ctc_blank=99)


def test_off_means_none():
    from frankenstein_amd.models.gpt2_model import GPT
    idx = torch.zeros((1, 2), dtype=torch.long)
    assert GPT._check_ctc(None, 0.0, None, None, 0, idx) is None
    assert GPT._check_ctc(torch.zeros((1, 5, 9)), 0.0, None, None, 0, idx) is None
    on = GPT._check_ctc(torch.zeros((5, 9)), 0.25, None, [4], 2, idx)
    assert on["blank"] == 8 and on["weight"] == 0.25 and on["from_prompt"] == 2 and on["logits"].shape == (1, 5, 9)
    assert on["lengths"].dtype == torch.int64 and on["lengths"].tolist() == [4]


@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def init(lib, logits=P, ldb=33 * 41, ldt=41, lens=P, S=3, T=33, C=41, blank=40, W=4, prompt=P, prompt_ld=1, n=1, row_lse=P, st0=P, psi=P, last=P, dtype=0):
    return lib.fk_ctc_prefix_init(logits, ldb, ldt, lens, S, T, C, blank, W, prompt, prompt_ld, n, row_lse, st0, psi, last, dtype, None)


def score(lib, logits=P, ldb=33 * 41, ldt=41, lens=P, row_lse=P, S=3, T=33, C=41, blank=40, W=4, k=20, top_lp=P, top_id=P, broadcast=0, weight=0.3,
          eos=7, fin=P, step=P, parent_log=P, tok_log=P, log_rows=5, st0=P, st1=2 * P, psi=P, last=P, dtype=0):
    return lib.fk_ctc_prefix_score(logits, ldb, ldt, lens, row_lse, S, T, C, blank, W, k, top_lp, top_id, broadcast, weight, eos, fin, step, parent_log,
                                   tok_log, log_rows, st0, st1, psi, last, dtype, None)


def test_exports_exist(lib):
    from frankenstein_amd import _lib
    for name in ("fk_ctc_prefix_init", "fk_ctc_prefix_score"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.CTC_PREFIX_FLOOR == R.FLOOR == float(f32(R.FLOOR))                        # the floor is an fp32 value


def test_entry_points_refuse_what_lies_outside_the_envelope(lib):
    msg = lambda: lib.fk_last_error()
    for fn in (init, score):
        assert fn(lib, dtype=2) == EINVAL and b"bad dtype" in msg()
        assert fn(lib, logits=None) == EINVAL and b"null pointer" in msg()
        assert fn(lib, T=1025, ldb=1025 * 41) == EINVAL and b"outside the envelope" in msg()
        assert fn(lib, T=0) == EINVAL
        assert fn(lib, W=17) == EINVAL and b"outside the envelope" in msg()
        assert fn(lib, W=0) == EINVAL
        assert fn(lib, C=1, blank=0) == EINVAL and b"C = 1" in msg()
        assert fn(lib, blank=41) == EINVAL and b"blank" in msg()
        assert fn(lib, ldt=40) == EINVAL and b"row stride" in msg()
        assert fn(lib, ldb=40) == EINVAL and b"row stride" in msg()
    assert init(lib, n=65, prompt_ld=65) == EINVAL and b"prompt labels" in msg()
    assert init(lib, prompt=None) == EINVAL and init(lib, prompt_ld=0) == EINVAL and init(lib, n=-1) == EINVAL
    assert init(lib, st0=None) == EINVAL and b"null pointer" in msg()
    assert score(lib, k=65) == EINVAL and b"k = 65" in msg()
    assert score(lib, k=0) == EINVAL
    for w in (-0.5, 1.5, float("nan")):
        assert score(lib, weight=w) == EINVAL and b"weight" in msg()
    assert score(lib, log_rows=0) == EINVAL and score(lib, st1=P) == EINVAL
    assert score(lib, fin=None) == EINVAL and b"finished flags" in msg()
    assert score(lib, step=None) == EINVAL and score(lib, top_id=None) == EINVAL and b"null pointer" in msg()


# =============================================================================================== the cases of the GPU file
@pytest.mark.parametrize("c", CC.ONE_STEP, ids=CC.one_id)
def test_one_step_cases_hold_what_they_are_for(c):
    """every planted case builds, its float32 restatement marks the same floor entries as float64, and the table as a whole holds every
    kind of entry the GPU test is about"""
    e = CC.one_step(c)
    assert e["tol"] >= 4 * e["err32"] and e["tol"] > 0 and np.isfinite(e["want"]).all()
    print(f"{CC.one_id(c)}: err32 = {e['err32']:.3g}, largest |psi| = {e['psi_max']:.4g}, tol = {e['tol']:.3g}, floor entries {int(e['floor'].sum())}")
    if c.k >= 4:
        live_rows = [q for q in range(e["top_id"].shape[0]) if not e["fin"][q * c.W if c.broadcast else q]]
        ids = e["top_id"][live_rows]
        assert (ids == e["blank"]).any() and (ids >= c.C).any() and (c.eos < 0 or (ids == c.eos).any())
        assert e["floor"].any() and (~e["floor"][live_rows]).any()


def test_one_step_table_covers_every_shape_and_variant():
    cs = CC.ONE_STEP
    assert {(c.S, c.W, c.k) for c in cs} == {(1, 1, 1), (1, 4, 20), (3, 4, 20), (2, 16, 64)}
    assert {c.T for c in cs} >= {1, 2, 33, 1024} and {c.C for c in cs} == {3, 41, 50258} and {c.dtype for c in cs} == {"f32", "bf16"}
    assert any(c.pad for c in cs) and any(c.lengths and 0 in c.lengths and c.T in c.lengths for c in cs) and any(c.broadcast for c in cs)
    assert {c.step % 2 for c in cs if c.step} == {0, 1}


@pytest.mark.parametrize("c", CC.LOOPS, ids=lambda c: f"T{c.T}")
def test_loop_salts_keep_every_decision_margin(c):
    """the float64 restatement's margins (W-th against (W+1)-th Gumbel key of every live beam, neighbours among the W + 1 best candidates) are
    all >= 1e-3 (tests/test_beam_gpu.py's threshold), no live row meets the floor, and the search spells the planted target"""
    e = CC.loop(c)
    print(f"T={c.T}: salt {CC.LOOP_SALT[c.T]}, smallest decision margin {e['margin']:.3g}")
    assert e["margin"] >= 1e-3
    best = int(np.argmax(e["final_scores"]))
    assert e["final_fin"][best] and e["final_seqs"][best] == list(c.target) + [CC.LOOP_EOS]
    frames = e["logits"].argmax(1)
    collapsed = [int(k) for k, _ in itertools.groupby(frames) if k != e["blank"]]
    assert collapsed == list(c.target)                     # what the greedy CTC decoder reads off the same logits
