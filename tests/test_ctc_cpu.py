"""CTC without a GPU: the float64 restatement (tests/ctc_ref.py) is pinned to torch's float64 CPU F.ctc_loss on every case of
tests/ctc_cases.py, the collapse reference to hand-written expectations, and the host side of the C ABI (route table, workspace size,
refusals before any launch) is exercised directly."""
import numpy as np
import pytest
import torch

from tests import ctc_cases as CC
from tests import ctc_ref as R

RTOL = 1e-10          # float64 against float64: only the order of the sums differs


@pytest.fixture(scope="module")
def built():
    from frankenstein_amd import build
    return build.build(verbose=False)


def _ref(case, zero_infinity):
    return R.ctc(case["logits"].numpy(), case["targets"].numpy(), case["input_lengths"].numpy(), case["target_lengths"].numpy(),
                 blank=case["blank"], zero_infinity=zero_infinity)


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_ref_equals_torch_float64(name):
    case = CC.make(name)
    ref = _ref(case, True)
    assert int(np.isinf(ref["raw"]).sum()) == case["infeasible"]
    want_none, grad = CC.torch_ctc(case, torch.float64, "none", True)
    np.testing.assert_allclose(ref["nll"], want_none.numpy(), rtol=RTOL, atol=0)
    # the gradient of the summed loss: probabilities and their differences, so the tolerance is relative to the tensor's scale
    g = R.dlogits(ref, "sum", 1.0)
    np.testing.assert_allclose(g, grad.numpy(), rtol=RTOL, atol=RTOL * np.abs(grad.numpy()).max())
    for reduction in ("sum", "mean"):
        want, gr = CC.torch_ctc(case, torch.float64, reduction, True)
        np.testing.assert_allclose(R.reduce(ref["nll"], ref["Lb"], reduction), want.numpy(), rtol=RTOL, atol=0)
        np.testing.assert_allclose(R.dlogits(ref, reduction, 1.0), gr.numpy(), rtol=RTOL, atol=RTOL * np.abs(gr.numpy()).max())
    # without zero_infinity a sample without alignment is +inf, the others are unchanged
    raw = _ref(case, False)["nll"]
    want_raw, _ = CC.torch_ctc(case, torch.float64, "none", False)
    assert np.array_equal(np.isinf(raw), np.isinf(want_raw.numpy())) and int(np.isinf(raw).sum()) == case["infeasible"]
    np.testing.assert_allclose(raw[np.isfinite(raw)], ref["nll"][np.isfinite(raw)], rtol=0, atol=0)


def test_ref_padding_gives_the_lengths():
    case = CC.make("a")
    assert np.array_equal(R.lengths_from_padding(case["targets"].numpy()), case["target_lengths"].numpy())
    a = R.ctc(case["logits"].numpy(), case["targets"].numpy(), case["input_lengths"].numpy(), None, blank=0)
    assert np.array_equal(a["nll"], _ref(case, False)["nll"])


def test_single_alignment_is_the_sum_along_it():
    """case a, sample 2: 2 2 3 3 in six frames has the one alignment 2 _ 2 3 _ 3"""
    case = CC.make("a")
    ref = R.ctc(case["logits"].numpy(), case["targets"].numpy(), case["input_lengths"].numpy(), case["target_lengths"].numpy(), blank=0)
    path = [2, 0, 2, 3, 0, 3]
    assert np.isclose(ref["nll"][2], -sum(ref["lp"][2, t, c] for t, c in enumerate(path)), rtol=1e-12, atol=0)


def test_lattice_product_is_the_loss_at_every_frame():
    case = CC.make("b32")
    ref = R.ctc(case["logits"].numpy(), case["targets"].numpy(), case["input_lengths"].numpy(), case["target_lengths"].numpy(),
                blank=case["blank"], want_lattice=True)
    for b, (alpha, beta) in enumerate(ref["lattice"]):
        ext = R.extended(case["targets"][b, :ref["Lb"][b]].numpy(), case["blank"])
        tb = int(ref["Tb"][b])
        tot = R.logsumexp(alpha + beta - ref["lp"][b, :tb][:, ext], axis=1)
        np.testing.assert_allclose(-tot, ref["nll"][b], rtol=1e-12)


_, A, B_ = 0, 1, 2


@pytest.mark.parametrize("frames,cut,want", [
    ([_, _, _], None, []),
    ([A, A, _, A, B_, B_], None, [A, A, B_]),
    ([A, _, A], None, [A, A]),
    ([A, A, _], None, [A]),
    ([A, A, _, A, B_, B_], 3, [A]),          # cut by input_lengths behind "a a _"
    ([A, B_, B_, A], 2, [A, B_]),
])
def test_collapse_reference(frames, cut, want):
    ids, lens = R.collapse(np.array([frames]), None if cut is None else [cut], blank=0, pad=-100)
    assert lens[0] == len(want) and list(ids[0, :len(want)]) == want and all(v == -100 for v in ids[0, len(want):])


def test_route_table(built):
    from frankenstein_amd import _lib
    from frankenstein_amd import kernels as K
    lib = _lib.lib()
    assert lib.fk_ctc_route(0) == _lib.CTC_WAVE and lib.fk_ctc_route(31) == _lib.CTC_WAVE
    assert lib.fk_ctc_route(32) == _lib.CTC_LDS and lib.fk_ctc_route(255) == _lib.CTC_LDS
    assert lib.fk_ctc_route(256) == -1 and b"envelope" in lib.fk_last_error()
    assert lib.fk_ctc_route(-1) == -1
    assert K.ctc_route(25) == _lib.CTC_WAVE and K.CTC_ROUTE_NAMES[K.ctc_route(120)] == "CTC_LDS"
    with pytest.raises(_lib.FrankenHipError, match="envelope"):
        K.ctc_route(256)


def test_workspace_grows_with_each_argument(built):
    from frankenstein_amd import _lib
    ws = _lib.lib().fk_ctc_workspace_bytes
    base = ws(4, 32, 25)
    assert base >= 2 * 4 * 32 * 64 * 4                 # the two lattices: [B, T, S_pad] fp32, S_pad = 64 at Lmax = 25
    assert ws(5, 32, 25) > base and ws(4, 33, 25) > base and ws(4, 32, 32) > base
    assert 0 < ws(4, 0, 25) < 4 * 64 * 4 * 4 + 4096     # without the lattice: the per-sample records only
    assert ws(4, 32, 256) == 0                          # outside the envelope


def test_refusals_need_no_gpu(built):
    """every refusal of fk_ctc_loss_fwd / _bwd / fk_ctc_collapse returns -1 with its message before any launch"""
    from frankenstein_amd import _lib
    lib = _lib.lib()
    P = 4096                                            # never dereferenced
    big = 1 << 30

    def fwd(logits=P, ldb=32 * 41, ldt=41, targets=P, nll=P, loss2=P, lse=P, B=2, T=32, C=41, Lmax=10, blank=0, reduction=_lib.CTC_MEAN,
            dtype=_lib.FK_F32, ws=P, nbytes=big):
        return lib.fk_ctc_loss_fwd(logits, ldb, ldt, targets, Lmax, None, None, -100, nll, loss2, lse, B, T, C, Lmax, blank, reduction, 1, 1,
                                   dtype, ws, nbytes, None)

    def bwd(logits=P, ldt=41, lse=P, gout=P, dl=P, lddt=41, C=41, Lmax=10, blank=0, dtype=_lib.FK_F32, ws=P, nbytes=big):
        return lib.fk_ctc_loss_bwd(logits, 32 * ldt, ldt, lse, gout, dl, 32 * lddt, lddt, 2, 32, C, Lmax, blank, _lib.CTC_MEAN, 1, dtype, ws,
                                   nbytes, None)

    for kw, msg in [(dict(logits=None), b"null pointer"), (dict(targets=None), b"null pointer"), (dict(nll=None), b"null pointer"),
                    (dict(loss2=None), b"null pointer"), (dict(lse=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(dtype=7), b"dtype"), (dict(C=1, ldt=41), b"C = 1"), (dict(blank=41), b"blank = 41"), (dict(blank=-1), b"blank = -1"),
                    (dict(Lmax=256), b"envelope"), (dict(ldt=40), b"row stride 40 below C"), (dict(reduction=3), b"reduction"),
                    (dict(nbytes=lib.fk_ctc_workspace_bytes(2, 32, 10) - 1), b"workspace too small")]:
        assert fwd(**kw) == -1 and msg in lib.fk_last_error(), (kw, lib.fk_last_error())
    for kw, msg in [(dict(logits=None), b"null pointer"), (dict(gout=None), b"null pointer"), (dict(dl=None), b"null pointer"),
                    (dict(ws=None), b"null pointer"), (dict(dtype=7), b"dtype"), (dict(C=1), b"C = 1"), (dict(blank=41), b"blank = 41"),
                    (dict(Lmax=256), b"envelope"), (dict(lddt=40), b"row stride"), (dict(ldt=40), b"row stride"),
                    (dict(nbytes=lib.fk_ctc_workspace_bytes(2, 32, 10) - 1), b"workspace too small")]:
        assert bwd(**kw) == -1 and msg in lib.fk_last_error(), (kw, lib.fk_last_error())
    assert lib.fk_ctc_collapse(None, 8, None, P, 8, P, 2, 8, 0, -100, None) == -1 and b"null pointer" in lib.fk_last_error()
    assert lib.fk_ctc_collapse(P, 7, None, P, 8, P, 2, 8, 0, -100, None) == -1 and b"strides" in lib.fk_last_error()
