"""CPU-side checks of the edit-distance family (csrc/editdist.hip): the restatement tests/edit_ref.py against the host yardstick
utils.metrics.edit_distance and against planted answers, its MBR and MWER parts against hand-computed values and central differences,
and, through the C ABI without a GPU, the envelope (FK_EINVAL before any launch) and the route function at every boundary."""
import numpy as np
import pytest
import torch

from frankenstein_amd.utils import metrics
from tests import edit_cases as EC
from tests import edit_ref as ER


@pytest.mark.parametrize("name", sorted(EC.DISTANCE))
def test_restatement_equals_the_host_metric(name):
    for explicit in ((True,) if name == "clamp" else (True, False)):
        c = EC.make_distance(name, explicit)
        a, b = c.a.tolist(), c.b.tolist()
        for g in range(len(b)):
            for h in range(c.n):
                ha = 0 if c.n_a == 1 else h
                if name == "clamp":
                    la = min(max(int(c.alen[g, ha]), 0), c.La)
                    lb = min(max(int(c.blen[g, h]), 0), c.Lb)
                    x, y = a[g][ha][:la], b[g][h][:lb]
                else:
                    x = ER.seq(a[g][ha], c.alen[g, ha] if explicit else None, EC.PAD)
                    y = ER.seq(b[g][h], c.blen[g, h] if explicit else None, EC.PAD)
                assert EC.PAD not in x and EC.PAD not in y
                assert metrics.edit_distance(x, y) == c.dist[g, h] and len(x) == c.alen_ref[g, ha]


def test_planted_answers():
    assert ER.distance(list(b"kitten"), list(b"sitting")) == 3
    assert ER.distance([], [5, 6, 7]) == 3 and ER.distance([5, 6, 7, 8], []) == 4 and ER.distance([], []) == 0
    assert ER.distance([1, 2, 3], [1, 2, 3]) == 0 and ER.distance([1, 2, 3], [4, 5]) == 3
    assert ER.distance([EC.BIG[0]], [EC.BIG[1]]) == 1                   # equal in the low 32 bits, different ids
    assert ER.seq([4, 5, -100, 6], None, -100) == [4, 5] and ER.seq([4, 5, -100, 6], 9, -100) == [4, 5, -100, 6] and ER.seq([4, 5], -2, -100) == []


def test_metric_properties_on_random_sequences():
    rng = np.random.default_rng(5)
    seqs = [[int(t) for t in rng.integers(0, 3, size=int(rng.integers(0, 9)))] for _ in range(12)]
    D = [[ER.distance(x, y) for y in seqs] for x in seqs]
    for i in range(12):
        assert D[i][i] == 0
        for j in range(12):
            assert D[i][j] == D[j][i] and abs(len(seqs[i]) - len(seqs[j])) <= D[i][j] <= max(len(seqs[i]), len(seqs[j]))
            for k in range(12):
                assert D[i][k] <= D[i][j] + D[j][k]


def test_mbr_on_a_hand_computed_list():
    """three hypotheses, scores ln 4, ln 2, ln 2 -> p = (1/2, 1/4, 1/4); dist rows (0 3 3), (3 0 1), (3 1 0): the risks are 1.5, 1.75,
    1.75, so the best-scored one wins; at scale 0 (p = 1/3 each) they are 2, 4/3, 4/3 and it drops to the last place; the tie of the other two
    goes to the smaller index.  A fourth, invalid hypothesis comes last with risk inf."""
    dist = [[0, 3, 3, -1], [3, 0, 1, -1], [3, 1, 0, -1], [-1, -1, -1, -1]]
    scores = np.array([np.log(4.0), np.log(2.0), np.log(2.0), -np.inf])
    risk, order, nv = ER.mbr(dist, scores, 1.0)
    np.testing.assert_allclose(risk[:3], [1.5, 1.75, 1.75], rtol=0, atol=1e-15)
    assert np.isinf(risk[3]) and list(order) == [0, 1, 2, 3] and nv == 3
    risk, order, nv = ER.mbr(dist, scores, 0.0)
    np.testing.assert_allclose(risk[:3], [2.0, 4.0 / 3.0, 4.0 / 3.0], rtol=0, atol=1e-15)
    assert list(order) == [1, 2, 0, 3]
    r32, o32, _ = ER.mbr(dist, scores, 1.0, np.float32)
    assert r32.dtype == np.float32 and list(o32) == [0, 1, 2, 3]
    assert ER.mbr(dist, np.full(4, -np.inf), 1.0)[2] == 0


@pytest.mark.parametrize("name", sorted(EC.RANKING))
def test_ranking_cases_keep_their_margin(name):
    c = EC.make_ranking(name)                                           # asserts gap >= 16 e32 and the planted properties
    assert c["gap"] >= EC.MARGIN * c["e32"]
    for b in range(c["B"]):
        assert sorted(c["order"][b]) == list(range(c["n"]))
        d = c["dist"][b]
        assert np.array_equal(d, d.T)


def test_mwer_combine_on_a_hand_computed_list():
    """nll = (ln 2, ln 4, ln 4) -> p = (1/2, 1/4, 1/4); errors (0, 2, 4): mean 2, loss = 1/2 (-2) + 1/4 (0) + 1/4 (2) = -1/2; d loss / d nll_i
    = -p_i (e_i - 1.5) = (0.75, -0.125, -0.625)"""
    nll = torch.tensor([np.log(2.0), np.log(4.0), np.log(4.0), 7.0], dtype=torch.float64, requires_grad=True)
    loss = ER.mwer_combine(nll, [0, 2, 4, 9], [True, True, True, False])
    loss.backward()
    assert abs(float(loss.detach()) + 0.5) < 1e-15
    np.testing.assert_allclose(nll.grad.numpy(), [0.75, -0.125, -0.625, 0.0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("nbest", [1, 4])
def test_mwer_gradient_against_central_differences(nbest):
    c = EC.make_mwer("small", nbest)
    args = (c.targets, c.target_lengths.numpy(), c.ids, c.lengths.numpy(), c.scores.numpy(), c.blank)
    loss, grad, nll, errors, valid = ER.mwer(c.logits, *args, ce_weight=0.3)
    assert np.isfinite(loss) and torch.isfinite(grad).all()
    if nbest == 4:
        assert not valid[0, 3] and not valid[1, 2] and np.isinf(nll[1, 2]) and not valid[2].any() and valid[0, :3].all()
    rng = np.random.default_rng(3)
    x = c.logits.double()
    for _ in range(6):
        b, t, k = (int(rng.integers(s)) for s in x.shape)
        h = 1e-6
        xp, xm = x.clone(), x.clone()
        xp[b, t, k] += h
        xm[b, t, k] -= h
        fd = (ER.mwer(xp, *args, ce_weight=0.3)[0] - ER.mwer(xm, *args, ce_weight=0.3)[0]) / (2 * h)
        assert abs(fd - float(grad[b, t, k])) < 1e-8 * max(1.0, abs(fd)), (b, t, k, fd, float(grad[b, t, k]))
    if nbest == 1:
        l0, g0, *_ = ER.mwer(c.logits, *args)
        assert l0 == 0.0 and float(g0.abs().max()) == 0.0


@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_envelope_is_refused_on_the_host(lib):
    """every violation returns FK_EINVAL (-1) before any GPU call: the pointers are never touched"""
    P = 4096                                                            # stands for a device pointer
    ed = lambda **k: lib.fk_edit_distance(*[{**dict(a=P, ldab=64, ldah=8, alen=None, n_a=4, La=8, b=P, ldbb=64, ldbh=8, blen=None, Lb=8, B=2, n=4,
                                                    pad=-100, dist=P, alen_out=None, stream=None), **k}[f] for f in
                                              ("a", "ldab", "ldah", "alen", "n_a", "La", "b", "ldbb", "ldbh", "blen", "Lb", "B", "n", "pad", "dist",
                                               "alen_out", "stream")])
    for bad in (dict(n=0, n_a=0), dict(n=33, n_a=33, ldab=8 * 33, ldbb=8 * 33), dict(La=0), dict(Lb=0), dict(La=1025, ldah=1025, ldab=4100),
                dict(Lb=1025, ldbh=1025, ldbb=4100), dict(ldah=7), dict(ldbh=7), dict(ldab=31), dict(ldbb=31), dict(n_a=2), dict(a=None),
                dict(b=None), dict(dist=None), dict(B=0)):
        assert ed(**bad) == -1 and b"fk_edit_distance" in lib.fk_last_error(), bad
    pw = lambda ids=P, ldb=64, ldh=8, lengths=P, B=2, n=4, T=8, dist=P: lib.fk_nbest_pairwise_distance(ids, ldb, ldh, lengths, None, B, n, T, dist, None)
    for bad in (dict(n=0), dict(n=33, ldb=8 * 33), dict(T=0), dict(T=1025, ldh=1025, ldb=4100), dict(ldh=7), dict(ldb=31), dict(ids=None),
                dict(lengths=None), dict(dist=None)):
        assert pw(**bad) == -1 and b"fk_nbest_pairwise_distance" in lib.fk_last_error(), bad

    def mbr(dist=P, scores=P, scale=1.0, ids=P, ldb=64, ldh=8, lengths=P, B=2, n=4, T=8, out=P, order=P):
        return lib.fk_mbr_rank(dist, scores, scale, ids, ldb, ldh, lengths, B, n, T, -100, out, out, out, out, out, order, out, None)
    for bad in (dict(n=0), dict(n=33, ldb=8 * 33), dict(T=0), dict(T=1025, ldh=1025, ldb=4100), dict(ldh=7), dict(scale=float("nan")),
                dict(scale=float("inf")), dict(dist=None), dict(scores=None), dict(ids=None), dict(lengths=None), dict(out=None), dict(order=None)):
        assert mbr(**bad) == -1 and b"fk_mbr_rank" in lib.fk_last_error(), bad
    mw = lambda nll=P, errors=P, B=2, n=4, loss=P, coef=P, count=P: lib.fk_mwer_combine(nll, errors, None, None, 255, B, n, loss, coef, count, None, None)
    for bad in (dict(n=0), dict(n=33), dict(B=0), dict(nll=None), dict(errors=None), dict(loss=None), dict(coef=None), dict(count=None)):
        assert mw(**bad) == -1 and b"fk_mwer_combine" in lib.fk_last_error(), bad
    rr = lambda rows=P, valid=P, out=P, B=2, n=4, E=8, dtype=0: lib.fk_mwer_reduce_rows(rows, valid, out, B, n, E, 0, dtype, None)
    for bad in (dict(n=0), dict(n=33), dict(B=0), dict(E=0), dict(rows=None), dict(valid=None), dict(out=None), dict(dtype=7)):
        assert rr(**bad) == -1 and b"fk_mwer_reduce_rows" in lib.fk_last_error(), bad


def test_route_boundaries(lib):
    from frankenstein_amd import _lib, kernels as K
    R = K.edit_distance_route
    assert R(1, 1) == R(64, 64) == R(64, 1024) == R(1024, 64) == R(1, 1024) == _lib.EDIT_LANE
    assert R(65, 65) == R(65, 1024) == R(256, 256) == R(1024, 256) == _lib.EDIT_ROWS4
    assert R(257, 257) == R(257, 1024) == R(1024, 1024) == _lib.EDIT_ROWS16
    for bad in ((0, 5), (5, 0), (1025, 5), (5, 1025)):
        with pytest.raises(_lib.FrankenHipError, match="fk_edit_distance_route"):
            R(*bad)
