"""CTC prefix beam search without a GPU: the float64 restatement (tests/ctc_beam_ref.py) is held to a brute-force enumeration of all
alignments where that is possible and to the CTC loss of its own results everywhere, and the host side of the C ABI (workspace query,
refusals before any launch) is exercised directly."""
import numpy as np
import pytest

from tests import ctc_beam_cases as BC
from tests import ctc_beam_ref as BR
from tests import ctc_ref as R

ALL = sorted(BC.CASES) + ["v_bf16"]


@pytest.fixture(scope="module")
def built():
    from frankenstein_amd import build
    return build.build(verbose=False)


def _exhaustive_inputs():
    """(label, logits [T, C], blank) with T <= 5, C <= 4: every sample of "x", the example "g", three more random ones"""
    out = []
    for name in ("x", "g"):
        case = BC.make(name)
        for b in range(case["logits"].shape[0]):
            out.append((f"{name}[{b}]", case["logits"][b, :int(case["input_lengths"][b])].numpy(), case["blank"]))
    rng = np.random.default_rng(11)
    for T, C, blank in ((5, 3, 1), (4, 4, 0), (3, 4, 3)):
        x = 2.0 * rng.standard_normal((T, C))
        x[:, blank] += 3.0
        out.append((f"random T={T} C={C}", x.astype(np.float32), blank))
    return out


@pytest.mark.parametrize("label,x,blank", _exhaustive_inputs(), ids=lambda v: v if isinstance(v, str) else "")
def test_ref_equals_brute_force(label, x, blank):
    """nothing pruned (K = C - 1, W = the number of labellings that exist; the restatement itself has no envelope): the same finite
    hypotheses, scores within 1e-12"""
    truth = {p: s for p, s in BR.brute_force(x, blank).items() if np.isfinite(s)}
    hyps, _, _ = BR.search_one(x, blank, max(32, len(truth)), x.shape[1] - 1, np.float64)
    got = dict(hyps)
    assert len(got) == len(hyps) and set(got) == set(truth), label
    for p, s in got.items():
        assert abs(s - truth[p]) <= 1e-12, (label, p, s, truth[p])
    assert [s for _, s in hyps] == sorted(got.values(), reverse=True)


def test_the_example():
    """blank 0.40, a 0.35, b 0.25 in both frames: the best path is blank blank, the best labelling is "a" with 0.4025"""
    case = BC.make("g")
    ref = case["ref"]
    assert ref["lengths"][0, 0] == 1 and ref["ids"][0, 0, 0] == 1 and list(ref["ids"][0, 0, 1:]) == [BC.PAD]
    assert abs(np.exp(ref["scores"][0, 0]) - 0.4025) < 1e-7            # the logits are fp32 logs of the probabilities
    ids, lens = BC.greedy(case["logits"].numpy(), case["input_lengths"].numpy(), 0)
    assert lens[0] == 0
    hyps = dict(ref["hyps"][0])
    assert abs(np.exp(hyps[()]) - 0.16) < 1e-7 and abs(np.exp(hyps[(2,)]) - 0.2625) < 1e-7
    assert ref["ties"][0] == [("frame", 1)] and list(ref["ids"][0, 3]) == [1, 2]    # "ab" and "ba" tie for the fourth place: 0.35 * 0.25 either way


@pytest.mark.parametrize("key", ALL)
def test_score_never_exceeds_the_loss(key):
    """a returned score is the mass of SOME alignments of that labelling: at most -nll of the CTC loss on the returned ids (+ 1e-9);
    absent slots are pad, length 0 and -inf"""
    case = BC.make(key)
    ref = case["ref"]
    x = case["logits"].numpy()
    B, nbest, T = ref["ids"].shape
    for h in range(nbest):
        have = np.isfinite(ref["scores"][:, h])
        assert np.all(ref["lengths"][~have, h] == 0) and np.all(ref["ids"][~have, h] == BC.PAD)
        loss = R.ctc(x, ref["ids"][:, h], case["input_lengths"].numpy(), ref["lengths"][:, h], blank=case["blank"], pad_value=BC.PAD)
        slack = ref["scores"][have, h] + loss["nll"][have]
        assert np.all(slack <= 1e-9), (key, h, slack)
    assert np.isfinite(ref["scores"][:, 0]).all()
    if key == "x":                                                   # nothing pruned: the score IS the log-probability
        have = np.isfinite(ref["scores"])
        for h in range(nbest):
            loss = R.ctc(x, ref["ids"][:, h], case["input_lengths"].numpy(), ref["lengths"][:, h], blank=case["blank"], pad_value=BC.PAD)
            np.testing.assert_allclose(ref["scores"][have[:, h], h], -loss["nll"][have[:, h]], rtol=0, atol=1e-12)


def test_cases_keep_their_purpose():
    """what the table of tests/ctc_beam_cases.py says each case is for"""
    s = BC.make("s")
    assert int(s["input_lengths"][2]) == 0 and s["ref"]["lengths"][2, 0] == 0 and s["ref"]["scores"][2, 0] == 0.0
    assert np.isneginf(s["ref"]["scores"][2, 1])
    assert all(len(h) <= 31 for h in BC.make("x")["ref"]["hyps"])
    for key in ("m", "l"):                                          # a resident prefix whose last label is no candidate of a frame
        case = BC.make(key)
        x, K = case["logits"].numpy(), case["K"]
        tb = int(case["input_lengths"][0])
        before, _, _ = BR.search_one(x[0, :tb - 1], case["blank"], case["W"], K)          # the beam that meets the last frame
        assert any(p and p[-1] not in BR.candidates(x[0, tb - 1], case["blank"], K) for p, _ in before), key
    assert BC.make("t")["ref"]["frame_gap"].max() < np.inf           # the table really overflows W = 32
    assert BC.make("l")["ref"]["lengths"][:, 0].min() > 20
    assert len(BC.make("v_bf16")["ref"]["ties"][0]) > 0 and BC.make("v")["ref"]["ties"] == [[], [], [], []]


def test_workspace_grows_with_each_argument(built):
    from frankenstein_amd import _lib
    ws = _lib.lib().fk_ctc_beam_workspace_bytes
    base = ws(4, 32, 5, 20)
    assert base >= 4 * 32 * (2 + 2 * 20) * 4 + 4 * (32 * 5 + 1) * 16   # per row: lse, lp[blank], K (lp, id); per sample T W + 1 nodes
    assert ws(5, 32, 5, 20) > base and ws(4, 33, 5, 20) > base and ws(4, 32, 6, 20) > base and ws(4, 32, 5, 21) > base
    assert ws(4, 32, 33, 20) == 0 and ws(4, 32, 5, 33) == 0 and ws(4, 32, 0, 20) == 0 and ws(4, 32, 5, 0) == 0 and ws(0, 32, 5, 20) == 0


def test_refusals_need_no_gpu(built):
    """every refusal of fk_ctc_beam_search returns -1 with its message before any launch"""
    from frankenstein_amd import _lib
    lib = _lib.lib()
    P = 4096                                            # never dereferenced
    big = 1 << 30

    def run(logits=P, ldb=32 * 41, ldt=41, B=2, T=32, C=41, blank=0, W=8, K=12, nbest=4, ids=P, ldib=4 * 32, ldih=32, lengths=P, scores=P,
            dtype=_lib.FK_F32, ws=P, nbytes=big):
        return lib.fk_ctc_beam_search(logits, ldb, ldt, None, B, T, C, blank, W, K, nbest, -100, ids, ldib, ldih, lengths, scores, dtype, ws,
                                      nbytes, None)

    for kw, msg in [(dict(logits=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(lengths=None), b"null pointer"),
                    (dict(scores=None), b"null pointer"), (dict(ws=None), b"workspace too small"), (dict(dtype=7), b"dtype"),
                    (dict(B=0), b"B = 0"), (dict(T=0), b"T = 0"), (dict(C=1), b"C = 1"), (dict(blank=41), b"blank = 41"),
                    (dict(blank=-1), b"blank = -1"), (dict(W=0), b"envelope"), (dict(W=33), b"envelope"), (dict(K=0), b"envelope"),
                    (dict(K=33), b"envelope"), (dict(nbest=0), b"nbest = 0"), (dict(nbest=9), b"nbest = 9"), (dict(ldt=40), b"row stride 40 below C"),
                    (dict(ldb=40), b"row stride"), (dict(ldih=31), b"ids strides"), (dict(ldib=3 * 32 + 31), b"ids strides"),
                    (dict(nbytes=lib.fk_ctc_beam_workspace_bytes(2, 32, 8, 12) - 1), b"workspace too small")]:
        assert run(**kw) == -1 and msg in lib.fk_last_error(), (kw, lib.fk_last_error())
