"""CPU-side checks of end-of-text aware decoding: fk_beam_select_eos, fk_beam_backtrack and fk_sample_topk_eos are exported and bound and
refuse what lies outside their envelope on the host (FK_EINVAL before any launch; the pointers are small fake addresses, so every call has
exactly one thing wrong with it), and the host form of the selection rule, gpt2_model._beam_step_host, equals the numpy restatement
`eos_step_ref` below exactly.  tests/test_eos_gpu.py holds the kernel to the same restatement."""
import ctypes

import numpy as np
import pytest
import torch

EINVAL = -1
P = 4096          # a fake, 16-byte aligned "device pointer": never dereferenced by a refused call


def lenpow_table(n, alpha):
    """fp32 [n]: 1 / L^alpha in float64, rounded once; entry 0 = 1"""
    L = np.arange(n, dtype=np.float64)
    L[0] = 1.0
    return (1.0 / L ** alpha).astype(np.float32)


def eos_step_ref(top_lp, top_id, broadcast, W, picks, scores, lens, fin, eos, table):
    """numpy restatement of one fk_beam_select_eos step of one sentence, given the draws picks[i] (entry numbers by draw rank).
    -> parent [W], token [W], scores fp32 [W] (raw), lens [W], fin [W], and the candidates in rank order as (norm, number, raw, L, token,
    parent) for the callers that measure margins"""
    f32 = np.float32
    cands = []
    for i in range(W):
        row = 0 if broadcast else i
        for r in range(W):
            if fin[i]:
                if r > 0:
                    continue                                                                      # a finished beam proposes itself once
                raw, L, tok = f32(scores[i]), int(lens[i]), int(eos)
            else:
                raw, L, tok = f32(f32(scores[i]) + f32(top_lp[row][picks[i][r]])), int(lens[i]) + 1, int(top_id[row][picks[i][r]])
            norm = f32(raw * table[min(max(L, 0), len(table) - 1)])
            cands.append((norm, i * W + r, raw, L, tok, i))
    cands.sort(key=lambda c: (-float(c[0]), c[1]))
    best = cands[:W]
    assert len(best) == W
    parent = [c[5] for c in best]
    tok = [c[4] for c in best]
    new_fin = [bool(fin[c[5]]) or (eos >= 0 and c[4] == eos) for c in best]
    return parent, tok, np.array([c[2] for c in best], f32), [c[3] for c in best], new_fin, cands


@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_exports_exist(lib):
    from frankenstein_amd import _lib
    h = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("fk_beam_select_eos", "fk_beam_backtrack", "fk_sample_topk_eos"):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    from frankenstein_amd import kernels as K
    assert callable(K.beam_select_eos) and callable(K.beam_backtrack) and callable(K.sample_topk_eos)


def select(lib, top_lp=P, top_id=P, row_stride=None, group_stride=None, S=3, W=5, k=20, scores=P, seed=P, step=P, pos=P, pos_inc=P, cur=P,
           parent_log=P, tok_log=P, log_rows=8, anc=P, anc_ld=320, ticket=P, eos=7, fin=P, len_=P, inv_lenpow=P, n_lenpow=10, live_acc=P, live=P):
    rs = k if row_stride is None else row_stride
    gs = W * k if group_stride is None else group_stride
    return lib.fk_beam_select_eos(top_lp, top_id, rs, gs, S, W, k, scores, seed, step, pos, pos_inc, cur, parent_log, tok_log, log_rows, anc, anc_ld,
                                  ticket, eos, fin, len_, inv_lenpow, n_lenpow, live_acc, live, None)


def test_beam_select_eos_refuses_bad_arguments(lib):
    for name in ("top_lp", "top_id", "scores", "seed", "step", "pos", "cur", "anc", "ticket", "fin", "len_", "inv_lenpow", "live_acc", "live"):
        assert select(lib, **{name: None}) == EINVAL and b"fk_beam_select_eos: null pointer" in lib.fk_last_error(), name
    for W, k in ((0, 20), (17, 20), (17, 64), (5, 4), (16, 15), (5, 65), (5, 0)):
        assert select(lib, W=W, k=k) == EINVAL and b"fk_beam_select_eos: need 1 <= W <= 16 and W <= k <= 64" in lib.fk_last_error(), (W, k)
    for n in (0, -1):
        assert select(lib, n_lenpow=n) == EINVAL and b"fk_beam_select_eos" in lib.fk_last_error() and b"n_lenpow" in lib.fk_last_error(), n
    assert select(lib, row_stride=19) == EINVAL and b"fk_beam_select_eos: rows overlap" in lib.fk_last_error()
    assert select(lib, group_stride=5 * 20 - 1) == EINVAL and b"fk_beam_select_eos: rows overlap" in lib.fk_last_error()
    assert select(lib, row_stride=0, group_stride=19) == EINVAL and b"fk_beam_select_eos: rows overlap" in lib.fk_last_error()
    assert select(lib, S=0) == EINVAL and b"fk_beam_select_eos" in lib.fk_last_error()
    assert select(lib, anc_ld=0) == EINVAL and b"fk_beam_select_eos" in lib.fk_last_error()
    assert select(lib, parent_log=None) == EINVAL and select(lib, tok_log=None) == EINVAL        # logs announced (log_rows = 8) but absent
    assert select(lib, log_rows=-1) == EINVAL


def backtrack(lib, parent_log=P, tok_log=P, log_rows=6, S=3, W=4, step=P, scores=P, len_=P, inv_lenpow=P, n_lenpow=10, out_ids=P, out_ld=9,
              out_cols=9, t0=2, pad=7, out_scores=P, out_len=P):
    return lib.fk_beam_backtrack(parent_log, tok_log, log_rows, S, W, step, scores, len_, inv_lenpow, n_lenpow, out_ids, out_ld, out_cols, t0, pad,
                                 out_scores, out_len, None)


def test_beam_backtrack_refuses_bad_arguments(lib):
    for name in ("parent_log", "tok_log", "step", "scores", "len_", "inv_lenpow", "out_ids", "out_scores", "out_len"):
        assert backtrack(lib, **{name: None}) == EINVAL and b"fk_beam_backtrack: null pointer" in lib.fk_last_error(), name
    for W in (0, 17):
        assert backtrack(lib, W=W) == EINVAL and b"fk_beam_backtrack: need 1 <= W <= 16" in lib.fk_last_error(), W
    assert backtrack(lib, S=0) == EINVAL and b"fk_beam_backtrack" in lib.fk_last_error()
    assert backtrack(lib, n_lenpow=0) == EINVAL and b"fk_beam_backtrack" in lib.fk_last_error() and b"n_lenpow" in lib.fk_last_error()
    assert backtrack(lib, log_rows=0) == EINVAL and b"fk_beam_backtrack" in lib.fk_last_error()
    assert backtrack(lib, out_cols=1, out_ld=9) == EINVAL and b"fk_beam_backtrack" in lib.fk_last_error() and b"prompt" in lib.fk_last_error()
    assert backtrack(lib, out_ld=8) == EINVAL and b"fk_beam_backtrack" in lib.fk_last_error()     # rows of 9 ids, 8 apart: they overlap
    assert backtrack(lib, t0=-1) == EINVAL and b"fk_beam_backtrack" in lib.fk_last_error()


def sample(lib, logits=P, ld=211, B=5, V=211, temperature=1.0, top_k=10, seed=P, step=P, pos_inc=P, cur=P, out=P, out_ld=8, out_cols=8, ticket=P,
           eos=7, done=P, len_=P, live_acc=P, live=P):
    return lib.fk_sample_topk_eos(logits, ld, B, V, temperature, top_k, seed, step, pos_inc, cur, out, out_ld, out_cols, ticket, eos, done, len_,
                                  live_acc, live, None)


def test_sample_topk_eos_refuses_bad_arguments(lib):
    for name in ("logits", "seed", "step", "cur", "ticket", "done", "len_", "live_acc", "live"):
        assert sample(lib, **{name: None}) == EINVAL and b"fk_sample_topk_eos: null pointer" in lib.fk_last_error(), name
    assert sample(lib, out_cols=0) == EINVAL and b"fk_sample_topk_eos" in lib.fk_last_error() and b"out_cols" in lib.fk_last_error()
    assert sample(lib, out_cols=9) == EINVAL and b"fk_sample_topk_eos" in lib.fk_last_error()     # wider than its row stride
    assert sample(lib, B=0) == EINVAL and b"fk_sample_topk_eos" in lib.fk_last_error()
    assert sample(lib, ld=210) == EINVAL and b"fk_sample_topk_eos" in lib.fk_last_error()
    assert sample(lib, V=1 << 31, ld=1 << 31) == EINVAL
    for t in (0.0, -1.0):
        assert sample(lib, temperature=t) == EINVAL and b"temperature" in lib.fk_last_error(), t


# =============================================================================================== the host rule
def _host(top_lp, top_id, picks, scores, lens, fin, eos, table):
    from frankenstein_amd.models.gpt2_model import _beam_step_host
    out = _beam_step_host(torch.from_numpy(top_lp), torch.from_numpy(top_id), torch.tensor(picks), torch.from_numpy(scores), torch.tensor(lens),
                          torch.tensor(fin), eos, torch.from_numpy(table))
    return [o.tolist() for o in out[:2]], out[2].numpy(), out[3].tolist(), out[4].tolist()


def _grid(rng, R, k):
    """rows of k distinct log-probabilities on a grid of 1/64, descending (tests/test_beam_gpu.py grid_rows)"""
    return np.stack([-np.sort(rng.choice(np.arange(1, 400), k, replace=False)).astype(np.float32) / 64 for _ in range(R)])


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("fin_kind", ["mixed", "all", "none"])
def test_beam_step_host_equals_the_numpy_restatement(alpha, fin_kind):
    """three chained steps, W = 4 of k = 10, ids from a 40-id range that holds eos, a table shorter than the lengths reach (the clamp)"""
    W, k, eos = 4, 10, 1007
    rng = np.random.default_rng(int(alpha * 10) + {"mixed": 100, "all": 200, "none": 300}[fin_kind])
    table = lenpow_table(6, alpha)
    scores = _grid(rng, 1, W)[0]
    lens = rng.integers(0, 5, W).tolist()
    fin = {"mixed": [False, True, False, True], "all": [True] * W, "none": [False] * W}[fin_kind]
    for t in range(3):
        top_lp = _grid(rng, W, k)
        top_id = np.stack([1000 + rng.choice(40, k, replace=False) for _ in range(W)]).astype(np.int64)
        picks = [rng.choice(k, W, replace=False).tolist() for _ in range(W)]
        parent, tok, want_scores, want_lens, want_fin, _ = eos_step_ref(top_lp, top_id, False, W, picks, scores, lens, fin, eos, table)
        (got_parent, got_tok), got_scores, got_lens, got_fin = _host(top_lp, top_id, picks, scores, lens, fin, eos, table)
        assert got_parent == parent and got_tok == tok and got_lens == want_lens and got_fin == want_fin, t
        assert np.array_equal(got_scores.view(np.uint32), want_scores.view(np.uint32)), t
        scores, lens, fin = want_scores, want_lens, want_fin
    if fin_kind == "all":
        assert tok == [eos] * W and fin == [True] * W and lens == got_lens


def test_beam_step_host_exact_ties_go_to_the_lower_candidate_number():
    """every beam holds the same score and the same row and draws the same entries: each candidate exists W times with exactly the same
    norm, and the survivors are the best entry from parents 0, 1, 2, 3; with a finished beam 1 (score 0: the best) its one candidate leads"""
    W, eos = 4, 9
    top_lp = np.tile(np.array([[-0.5, -1.0, -2.0, -4.0]], np.float32), (W, 1))
    top_id = np.tile(np.array([[11, 22, 33, 44]], np.int64), (W, 1))
    picks = [[0, 1, 2, 3]] * W
    for alpha in (0.0, 1.0):
        table = lenpow_table(8, alpha)
        scores, lens = np.full(W, -1.0, np.float32), [2] * W
        for fin in ([False] * W, [False, True, False, False]):
            sc = scores.copy()
            if fin[1]:
                sc[1] = 0.0
            want = eos_step_ref(top_lp, top_id, False, W, picks, sc, lens, fin, eos, table)
            (parent, tok), got_scores, got_lens, got_fin = _host(top_lp, top_id, picks, sc, lens, fin, eos, table)
            assert (parent, tok, got_lens, got_fin) == (want[0], want[1], want[3], want[4])
            assert np.array_equal(got_scores, want[2])
            if fin[1]:
                assert parent == [1, 0, 2, 3] and tok == [eos, 11, 11, 11] and got_fin == [True, False, False, False] and got_lens == [2, 3, 3, 3]
            else:
                assert parent == [0, 1, 2, 3] and tok == [11] * 4 and got_lens == [3] * 4


def test_beam_step_host_without_an_eos_is_the_plain_rule():
    """eos = -1, nothing finished, a table of ones: the W best of scores + lp, stable"""
    W, k = 4, 10
    rng = np.random.default_rng(5)
    top_lp, scores = _grid(rng, W, k), _grid(rng, 1, W)[0]
    top_id = np.stack([rng.choice(50257, k, replace=False) for _ in range(W)]).astype(np.int64)
    picks = [rng.choice(k, W, replace=False).tolist() for _ in range(W)]
    (parent, tok), got_scores, lens, fin = _host(top_lp, top_id, picks, scores, [0] * W, [False] * W, -1, lenpow_table(4, 0.0))
    cand = (torch.from_numpy(scores)[:, None] + torch.from_numpy(top_lp).gather(1, torch.tensor(picks))).reshape(-1)
    order = torch.sort(cand, descending=True, stable=True).indices[:W]
    assert parent == (order // W).tolist() and np.array_equal(got_scores, cand[order].numpy()) and lens == [1] * W and fin == [False] * W


def test_beam_state_defaults_allocate_nothing_new():
    from frankenstein_amd import kernels as K
    st = K.BeamState("cpu", 4, 6, 32, seed=1)
    for name in ("fin", "len", "inv_lenpow", "live_acc", "live", "eos", "length_penalty"):
        assert not hasattr(st, name), name
    assert sorted(vars(st)) == ["anc", "groups", "parent_log", "scores", "seed", "step", "ticket", "tok_log", "width"]
    assert sorted(k for k, v in vars(st).items() if torch.is_tensor(v)) == ["anc", "parent_log", "scores", "seed", "step", "ticket", "tok_log"]
    for kw in (dict(eos=7), dict(length_penalty=0.6), dict(eos=7, length_penalty=1.0)):
        st = K.BeamState("cpu", 4, 6, 32, seed=[1, 2], groups=2, **kw)
        assert st.fin.shape == st.len.shape == (8,) and st.fin.dtype == st.len.dtype == torch.int32 and int(st.fin.sum()) == 0
        assert st.live_acc.numel() == st.live.numel() == 1 and int(st.live_acc) == 0
        alpha = kw.get("length_penalty", 0.0)
        assert st.inv_lenpow.dtype == torch.float32 and st.inv_lenpow.numel() >= 6 + 1
        assert np.array_equal(st.inv_lenpow.numpy(), lenpow_table(st.inv_lenpow.numel(), alpha))
    assert np.array_equal(K.inv_lenpow_table(5, 0.0).numpy(), np.ones(5, np.float32))
