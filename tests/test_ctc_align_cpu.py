"""CTC forced alignment without a GPU: the float64 restatement tests/ctc_align_ref.py against enumeration, the cases the GPU tests run
against it (that they are decisive: the same recursion in float32 finds the same path; that a planted alignment is found), and the
host-side refusals of fk_ctc_align."""
import numpy as np
import pytest
import torch

from tests import ctc_align_ref as A
from tests import ctc_cases as CC
from tests import ctc_ref as R


def _tiny_samples():
    """(name, lp-producing logits [T, C], labels, blank): T <= 7, C <= 4, L <= 3"""
    rng = np.random.default_rng(11)
    out = []
    for T, C, labels, blank in [(5, 4, [1, 2, 3], 0), (7, 4, [2, 2, 1], 0), (6, 3, [1, 1, 1], 2), (4, 4, [], 3), (3, 3, [0], 1), (7, 4, [3, 1, 3], 0),
                                (1, 3, [2], 0), (5, 2, [0, 0, 0], 1), (2, 4, [1, 2, 3], 0), (3, 3, [1, 1], 0)]:
        for rep in range(3):
            out.append((f"rand T{T} {labels} #{rep}", 3.0 * rng.standard_normal((T, C)), labels, blank))
        out.append((f"flat T{T} {labels}", np.zeros((T, C)), labels, blank))                      # every alignment ties exactly
        two = np.zeros((T, C))
        two[::2, blank] = 1.0                                                                   # ties between groups of alignments
        out.append((f"steps T{T} {labels}", two, labels, blank))
    return out


@pytest.mark.parametrize("sample", _tiny_samples(), ids=lambda s: s[0])
def test_restatement_equals_enumeration(sample):
    """score, and the PATH the tie rules name, not merely an optimal one"""
    _, x, labels, blank = sample
    T, C = x.shape
    tg = np.array([labels + [CC.PAD] * (3 - len(labels))], dtype=np.int64)
    got = A.viterbi(x[None], tg, None, None, blank)
    ext = R.extended(np.array(labels, dtype=np.int64), blank)
    score, states = A.brute_force(got["lp"][0], ext)
    feasible = T >= len(labels) + CC.repeats(labels)
    assert (states is not None) == feasible
    if not feasible:
        assert got["score"][0] == -np.inf and got["states"][0] is None
        assert (got["path"] == -100).all() and (got["index"] == -1).all() and (got["start"] == -1).all() and (got["end"] == -1).all()
        assert not got["label_lp"].any()
        return
    assert got["score"][0] == score
    assert np.array_equal(got["states"][0], states), (got["states"][0], states)
    # the rows follow from the states
    L = len(labels)
    assert R.collapse(got["path"], None, blank)[0][0, :L].tolist() == labels
    for i in range(L):
        s, e = got["start"][0, i], got["end"][0, i]
        assert e > s and (got["index"][0, s:e] == i).all() and (got["path"][0, s:e] == labels[i]).all()
        assert got["label_lp"][0, i] == pytest.approx(got["lp"][0, s:e, labels[i]].sum(), abs=1e-12)
    assert (got["start"][0, L:] == -1).all() and (got["end"][0, L:] == -1).all() and not got["label_lp"][0, L:].any()
    assert ((got["index"][0] >= 0).sum() == (got["end"][0, :L] - got["start"][0, :L]).sum())


def test_empty_sample_and_length_clamps():
    x = np.zeros((3, 4, 3))
    tg = np.array([[1, 2], [CC.PAD, CC.PAD], [1, 1]], dtype=np.int64)
    got = A.viterbi(x, tg, np.array([0, 0, 9]), np.array([2, 0, 7]), 0)
    assert got["score"][0] == -np.inf and got["score"][1] == 0.0 and np.isfinite(got["score"][2])
    assert (got["path"][:2] == -100).all() and (got["index"][:2] == -1).all()
    assert got["Tb"].tolist() == [0, 0, 4] and got["Lb"].tolist() == [2, 0, 2]
    # a label past the classes and a label equal to the blank take the loss's clamp
    _, _, lab = A.clamp_inputs(np.array([[7, 0, -3]]), 4, 3, None, None, 0)
    assert lab.tolist() == [[2, 1, 1]]
    _, _, lab = A.clamp_inputs(np.array([[7, 2, -3]]), 4, 3, None, None, 2)
    assert lab.tolist() == [[1, 1, 0]]


def _f64_f32(c, bf16=False):
    x = c["logits"].to(torch.bfloat16).float() if bf16 else c["logits"]
    args = (x.numpy(), c["targets"].numpy(), c["input_lengths"].numpy(), c["target_lengths"].numpy(), c["blank"])
    return A.viterbi(*args), A.viterbi(*args, dtype=np.float32)


@pytest.mark.parametrize("key", A.NAMES + ["c_bf16"])
def test_cases_are_decisive(key):
    """the recursion in float32 finds exactly the float64 path on every case: no case holds a near-tie that an fp32 kernel may resolve
    the other way (case c: score error of the float32 run at most 1.1e-3 at |score| ~ 3e3)"""
    name, bf16 = (key[:-5], True) if key.endswith("_bf16") else (key, False)
    c = A.case(name)
    r64, r32 = _f64_f32(c, bf16)
    assert int(np.isinf(r64["score"]).sum()) == c["infeasible"]
    for k in ("path", "index", "start", "end"):
        assert np.array_equal(r64[k], r32[k]), (key, k)
    fin = np.isfinite(r64["score"])
    err = float(np.abs(r32["score"].astype(np.float64)[fin] - r64["score"][fin]).max())
    print(f"ctc align {key}: |float32 - float64| score {err:.3e} at max |score| {np.abs(r64['score'][fin]).max():.1f}")
    assert np.array_equal(np.isinf(r32["score"]), np.isinf(r64["score"]))
    T = c["logits"].shape[1]                             # a chain of T fp32 adds of fp32-rounded terms: at most (T + 8) ulp of the largest partial sum
    assert err <= (T + 8) * 2.0 ** -23 * max(1.0, float(np.abs(r64["score"][fin]).max()))
    nll = R.ctc(c["logits"].to(torch.bfloat16).float().numpy() if bf16 else c["logits"].numpy(), c["targets"].numpy(), c["input_lengths"].numpy(),
                c["target_lengths"].numpy(), blank=c["blank"])["raw"]
    assert np.all(r64["score"][fin] <= -nll[fin] + 1e-9) and np.array_equal(np.isinf(nll), ~fin)


@pytest.mark.parametrize("key", A.NAMES)
def test_planted_alignment_is_found(key):
    c = A.planted(key)
    for bf16 in (False, True):
        r64, r32 = _f64_f32(c, bf16)
        assert sum(s is None for s in c["planted"]) == c["infeasible"]
        for b, st in enumerate(c["planted"]):
            if st is None:
                assert r64["states"][b] is None and r64["score"][b] == -np.inf
            else:
                assert np.array_equal(r64["states"][b], st), (key, b)
        for k in ("path", "index", "start", "end"):
            assert np.array_equal(r64[k], r32[k]), (key, k)


# ---- the C ABI refuses on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _align(lib, **over):
    """a call whose arguments are all inside the envelope (pointers are never followed: the refusals come before any launch)"""
    from frankenstein_amd import _lib
    B, T, C, Lmax = 2, 40, 7, 5
    a = dict(logits=16, ldb=T * C, ldt=C, targets=16, ldtgt=Lmax, il=None, tl=None, pad_value=-100, B=B, T=T, C=C, Lmax=Lmax, blank=0, pad=-100,
             score=16, path=16, ld_path=T, index=16, ld_index=T, start=16, end=16, label_lp=16, ld_lab=Lmax, dtype=_lib.FK_F32, ws=16, ws_bytes=None,
             stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.fk_ctc_align_workspace_bytes(a["B"], a["T"], min(a["Lmax"], 255))
    return lib.fk_ctc_align(*a.values())


def test_host_side_refusals(lib):
    assert lib.fk_ctc_align_workspace_bytes(2, 40, 5) >= 2 * 40 * 4 + 2 * 3 * 64 * 4
    for B, T, L in ((0, 40, 5), (2, 0, 5), (2, 40, 256), (2, 40, -1), (1 << 20, 1 << 12, 5)):
        assert lib.fk_ctc_align_workspace_bytes(B, T, L) == 0
    for over, msg in ((dict(Lmax=256, ldtgt=256, ld_lab=256), b"Lmax = 256"), (dict(ld_path=39), b"stride 39"), (dict(ld_index=39), b"stride"),
                      (dict(ld_lab=4), b"label stride 4"), (dict(score=None), b"null pointer"), (dict(path=None), b"null pointer"),
                      (dict(ws_bytes=lib.fk_ctc_align_workspace_bytes(2, 40, 5) - 1), b"workspace too small"), (dict(dtype=7), b"dtype"),
                      (dict(blank=7), b"blank"), (dict(ldt=6), b"row stride")):
        assert _align(lib, **over) == -1, over
        assert msg in lib.fk_last_error(), (over, lib.fk_last_error())


def test_python_constants_mirror_the_kernel():
    import re
    from pathlib import Path
    from frankenstein_amd import kernels as K
    src = (Path(K.__file__).parent / "csrc" / "ctc.hip").read_text()
    assert int(re.search(r"constexpr int CTC_ALIGN_PACK = (\d+);", src).group(1)) == K.CTC_ALIGN_PACK == A.PACK
    assert int(re.search(r"constexpr int CTC_ALIGN_CHUNK = (\d+);", src).group(1)) == K.CTC_ALIGN_CHUNK == A.CHUNK
