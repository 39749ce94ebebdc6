"""Cached beam search on the MI355X: the three kernels (fk_attn_decode_beam, fk_beam_topk, fk_beam_select) against float64 / numpy
restatements written here, and GPT.generate_beam_search / GPT.beam_search with use_cache=True against the reference's recorded tokens and
against the re-forward path they replace.

Tolerances: attention as tests/test_envelope_gpu.py holds fk_attn_decode (close() defaults in fp32, atol 2e-2 in bf16); log-probabilities
1e-4, the project's fp32 logit tolerance; everything fk_beam_select writes is compared exactly (its scores are single fp32 additions, its
keys are only compared where they are >= 1e-3 apart, far above an ulp of logf)."""
import math

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from tests import cases as C
from tests.sample_ref import philox4x32_10
from tests.test_decode_gpt2_gpu import inputs as inputs_124m
from tests.test_decode_gpt2_gpu import model, z  # noqa: F401  (module-scoped fixtures: GPT-2 124M and its golden file)
from tests.test_kernels_gpu import close, dev, q, rnd
from tests.test_models_gpu import load_synth, mk_gpt

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
TMAX = 320


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


@pytest.fixture
def fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def i32(x):
    return torch.tensor([x], dtype=torch.int32, device="cuda")


# =============================================================================================== 1. fk_attn_decode_beam
def _beam_attn_ref(qkv, kv, anc, pos, H, D):
    """float64: beam b's row j < pos comes from slot anc[b, j], row pos from slot b -> [W, d]"""
    W, d = qkv.shape[0], H * D
    slot = torch.cat([anc[:, :pos].long(), torch.arange(W)[:, None]], 1)                          # [W, pos + 1]
    rows = kv[slot, torch.arange(pos + 1)[None, :]].double()                                      # [W, pos + 1, 2d]
    kh = rows[..., :d].view(W, pos + 1, H, D).transpose(1, 2)
    vh = rows[..., d:].view(W, pos + 1, H, D).transpose(1, 2)
    p = torch.softmax((qkv[:, :d].double().view(W, H, 1, D) @ kh.transpose(-1, -2)) / math.sqrt(D), -1)
    return (p @ vh).view(W, d)


def _beam_attn_case(W, D, pos, dtype, H=2):
    d = H * D
    g = torch.Generator().manual_seed(1000 * W + 10 * D + pos)
    qkv = q(rnd(W, 3 * d, seed=pos + 1), dtype)
    kv = q(rnd(W, TMAX, 2 * d, seed=pos + 2), dtype)
    anc = torch.randint(0, W, (W, TMAX), generator=g, dtype=torch.int32)
    used = torch.zeros(W, TMAX, dtype=torch.bool)
    used[anc[:, :pos].long().reshape(-1), torch.arange(pos).repeat(W)] = True
    used[torch.arange(W), pos] = True
    kv[~used] = float("nan")                                                                      # a row no ancestry entry points to stays poison
    anc[:, pos:] = 7 * W + 3                                                                      # never read: the row pos is the beam's own
    return qkv, kv, anc


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_attn_decode_beam_against_float64_gather_softmax(K, dtype, D):
    """H = 2, W in {1, 5, 16}, *pos in {0, 1, 255, 256, 299} (one key; a partial trip; both sides of 256 keys), random ancestry, every cache
    row outside the ancestry NaN: the output is finite and equals the float64 gather + softmax"""
    for W in (1, 5, 16):
        for pos in (0, 1, 255, 256, 299):
            qkv, kv, anc = _beam_attn_case(W, D, pos, dtype)
            got = K.attn_decode_beam(dev(qkv, dtype), dev(kv, dtype), dev(anc), i32(pos), 2)
            assert bool(torch.isfinite(got).all()), (W, pos)
            want = _beam_attn_ref(qkv, kv, anc, pos, 2, D)
            print(f"attn_decode_beam W={W} D={D} {dtype} pos={pos}: max |o - f64| = {float((got.double().cpu() - want).abs().max()):.3g}")
            close(got, want, dtype, **({} if dtype == torch.float32 else {"atol16": 2e-2}))


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_attn_decode_beam_identity_ancestry_is_attn_decode(K, dtype, D):
    W, H = 5, 2
    for pos in (0, 255, 256, 299):
        qkv, kv = dev(rnd(W, 3 * H * D, seed=pos + 1), dtype), dev(rnd(W, TMAX, 2 * H * D, seed=pos + 2), dtype)
        kv[:, pos + 1:] = float("nan")
        anc = torch.arange(W, dtype=torch.int32, device="cuda")[:, None].repeat(1, TMAX).contiguous()
        got = K.attn_decode_beam(qkv, kv, anc, i32(pos), H)
        close(got, K.attn_decode(qkv, kv, i32(pos), H), dtype, **({} if dtype == torch.float32 else {"atol16": 2e-2}))


def test_attn_decode_beam_clamps_a_corrupt_table(K):
    """entries outside [0, W) read the rows the clamped entries name (bit for bit), never anything outside the cache"""
    W, H, D, pos = 5, 2, 64, 40
    qkv, kv = dev(rnd(W, 3 * H * D, seed=1), torch.bfloat16), dev(rnd(W, TMAX, 2 * H * D, seed=2), torch.bfloat16)
    anc = torch.randint(-2 ** 31, 2 ** 31 - 1, (W, TMAX), generator=torch.Generator().manual_seed(3), dtype=torch.int64).to(torch.int32)
    anc[:, ::3] = torch.randint(0, W, (W, len(range(0, TMAX, 3))), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    got = K.attn_decode_beam(qkv, kv, dev(anc), i32(pos), H)
    want = K.attn_decode_beam(qkv, kv, dev(anc.clamp(0, W - 1)), i32(pos), H)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


# =============================================================================================== 2. fk_beam_topk
@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("R,V,k", [(1, 211, 1), (5, 211, 20), (3, 50257, 64), (16, 50257, 20)])
def test_beam_topk_against_float64_log_softmax(K, R, V, k, temperature):
    buf = rnd(R, V + 3, seed=V + k, scale=3.0)                                                     # row stride V + 3: ld > V
    logits = buf[:, :V]
    want_lp, want_id = torch.log_softmax(logits.double() / temperature, -1).topk(k, -1)
    got_lp, got_id = K.beam_topk(dev(buf)[:, :V], temperature, k)
    assert got_lp.shape == (R, k) and got_id.dtype == torch.int64
    assert torch.equal(got_id.cpu(), want_id)
    err = float((got_lp.double().cpu() - want_lp).abs().max())
    print(f"beam_topk R={R} V={V} k={k} T={temperature}: max |lp - f64| = {err:.3g}")
    assert err <= 1e-4


def test_beam_topk_ties_keep_the_lowest_ids_in_ascending_order(K):
    # two values above the tie, the tie (2.0 at six ids) straddles rank 5: its three lowest ids come out, ascending
    x = rnd(1, 211, seed=5).clamp(max=1.0)
    x[0, [200, 3, 77, 150, 9, 42]] = 2.0
    x[0, 100], x[0, 5] = 3.0, 2.5
    lp, ids = K.beam_topk(dev(x), 1.0, 5)
    assert ids.cpu().tolist() == [[100, 5, 3, 9, 42]]
    want = torch.log_softmax(x.double(), -1)[0, [100, 5, 3, 9, 42]]
    assert float((lp.double().cpu()[0] - want).abs().max()) <= 1e-4
    # the same across the whole 50257-wide row (ties in many threads' chunks), two rows with different tie sets, k inside the tie from rank 1
    x = rnd(2, 50257, seed=6).clamp(max=1.0)
    t0, t1 = [50000, 17, 30000, 1024, 49, 2048, 50256], [40000, 0, 12345, 12346]
    x[0, t0], x[1, t1] = 4.0, 4.0
    lp, ids = K.beam_topk(dev(x), 0.7, 3)
    assert ids.cpu().tolist() == [sorted(t0)[:3], sorted(t1)[:3]]
    # every value equal: ids 0 .. k-1, lp = -log V
    lp, ids = K.beam_topk(torch.zeros(2, 211, device="cuda"), 1.0, 20)
    assert ids.cpu().tolist() == [list(range(20))] * 2
    assert float((lp.cpu() + math.log(211)).abs().max()) <= 1e-5
    # k = V
    x = rnd(1, 7, seed=8)
    lp, ids = K.beam_topk(dev(x), 1.0, 7)
    assert ids.cpu().tolist() == [torch.argsort(x[0], descending=True).tolist()]


# =============================================================================================== 3. fk_beam_select
def test_philox_restatement_known_answers():
    """the known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10 rounds)"""
    assert philox4x32_10((0, 0), (0, 0, 0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def select_ref(top_lp, top_id, broadcast, W, scores, seed, step, pos, anc):
    """numpy restatement of fk_beam_select.  -> parent [W], cur [W], scores [W] fp32, the updated table, the margins (the smallest gap
    between the W-th and (W+1)-th Gumbel key of a beam; the smallest non-zero gap between neighbours among the W + 1 best candidate
    scores: equal scores fall under the tie rule, which is exact on both sides) and the draws pick[i] (entry numbers by draw rank)"""
    f32 = np.float32
    k = top_lp.shape[1]
    pick, key_margin = [], np.inf
    for i in range(W):
        row = top_lp[0 if broadcast else i]
        keys = np.empty(k, f32)
        for j in range(k):
            c0 = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (step & 0xFFFFFFFF, step >> 32, i, 0xBEA30000 | j))[0]
            u = (f32(c0 >> 8) + f32(0.5)) * f32(1.0 / 16777216.0)
            keys[j] = row[j] - np.log(-np.log(u, dtype=f32), dtype=f32)
        order = sorted(range(k), key=lambda j: (-keys[j], j))
        if k > W:
            key_margin = min(key_margin, float(keys[order[W - 1]] - keys[order[W]]))
        pick.append(order[:W])
    cand = [(f32(scores[i] + top_lp[0 if broadcast else i][pick[i][r]]), i, r) for i in range(W) for r in range(W)]
    order = sorted(range(W * W), key=lambda c: (-cand[c][0], c))
    best = [float(cand[c][0]) for c in order[:W + 1]]
    gaps = [a - b for a, b in zip(best, best[1:]) if a != b]
    parent = [cand[c][1] for c in order[:W]]
    cur = [int(top_id[0 if broadcast else cand[c][1]][pick[cand[c][1]][cand[c][2]]]) for c in order[:W]]
    new_scores = np.array([cand[c][0] for c in order[:W]], f32)
    new_anc = anc.copy()
    if pos >= 0:
        old = anc[:, :pos + 1].copy()
        old[:, pos] = np.arange(W)
        new_anc[:, :pos + 1] = old[parent]
    return parent, cur, new_scores, new_anc, key_margin, (min(gaps) if gaps else np.inf), pick


def grid_rows(rng, R, k):
    """R rows of k distinct log-probabilities on a grid of 1/64, descending: every candidate score is then an exact multiple of 1/64,
    so two candidates either tie exactly or lie >= 0.0156 apart"""
    return np.stack([-np.sort(rng.choice(np.arange(1, 400), k, replace=False)).astype(np.float32) / 64 for _ in range(R)])


@pytest.mark.parametrize("broadcast", [False, True], ids=["row_stride=k", "row_stride=0"])
@pytest.mark.parametrize("W,k", [(1, 1), (1, 20), (4, 4), (4, 20), (16, 16), (16, 20)])
def test_beam_select_three_steps_against_numpy(K, W, k, broadcast):
    """three consecutive steps on one state, from *pos = 254 (the columns 0 .. 256 of the table: one and two trips of the 256 threads):
    parents, tokens, scores, both logs, the whole table, the step counter and the position, all exact"""
    rng = np.random.default_rng(100 * W + k)
    seed, pos0, steps, log_rows = 0x1234_5678_9ABC_DEF0 + W, 254, 3, 2                              # the logs hold two of the three steps
    st = K.BeamState("cuda", W, log_rows, TMAX, seed=seed)
    anc = rng.integers(0, W, (W, TMAX)).astype(np.int32)
    st.anc.copy_(torch.from_numpy(anc))
    st.scores.copy_(torch.from_numpy(grid_rows(rng, 1, W)[0]))
    st.parent_log.fill_(-5)
    st.tok_log.fill_(-5)
    scores = st.scores.cpu().numpy()
    cur, pos = torch.empty(W, dtype=torch.int64, device="cuda"), i32(pos0)
    for t in range(steps):
        top_lp = grid_rows(rng, W, k)
        top_id = np.stack([rng.choice(50257, k, replace=False) for _ in range(W)]).astype(np.int64)
        parent, want_cur, scores, anc, key_margin, score_margin, _ = select_ref(top_lp, top_id, broadcast, W, scores, seed, t, pos0 + t, anc)
        print(f"W={W} k={k} step {t}: Gumbel key margin {key_margin:.3g}, candidate score margin {score_margin:.3g}")
        assert key_margin >= 1e-3 and score_margin >= 1e-3
        K.beam_select(dev(torch.from_numpy(top_lp)), dev(torch.from_numpy(top_id)), st, cur, pos, pos_inc=pos, broadcast=broadcast)
        assert cur.cpu().tolist() == want_cur, t
        assert np.array_equal(st.scores.cpu().numpy(), scores), t
        assert np.array_equal(st.anc.cpu().numpy(), anc), t
        assert int(st.step) == t + 1 and int(pos) == pos0 + t + 1
        if t < log_rows:
            assert st.parent_log[t].cpu().tolist() == parent and st.tok_log[t].cpu().tolist() == want_cur, t
    assert st.parent_log.shape[0] == log_rows                                                      # the third step wrote no log row (and no guard band: conftest)


def test_beam_select_exact_ties_go_to_the_lower_parent(K):
    """a broadcast row with k = W: every beam proposes every entry, so each candidate exists W times with exactly the same score.  The
    survivors are the best entry from parents 0, 1, 2, 3, whatever the draw; a negative *pos leaves the table alone"""
    W = 4
    st = K.BeamState("cuda", W, 1, TMAX, seed=7)
    st.anc.fill_(3)
    top_lp = torch.tensor([[-0.5, -1.0, -2.0, -4.0]], device="cuda")
    top_id = torch.tensor([[11, 22, 33, 44]], device="cuda")
    cur = torch.empty(W, dtype=torch.int64, device="cuda")
    K.beam_select(top_lp, top_id, st, cur, i32(-1), broadcast=True)
    assert cur.cpu().tolist() == [11] * 4 and st.parent_log[0].cpu().tolist() == [0, 1, 2, 3]
    assert st.scores.cpu().tolist() == [-0.5] * 4 and bool((st.anc == 3).all()) and int(st.step) == 1
    # unequal beam scores: parent 2 leads, then the tie of parents 0 and 1 at -1.5 (0 first), then parent 2's second entry
    st.scores.copy_(torch.tensor([-1.0, -1.0, 0.0, -9.0]))
    K.beam_select(top_lp, top_id, st, cur, i32(5), broadcast=True)
    assert st.parent_log.shape[0] == 1 and int(st.step) == 2
    assert cur.cpu().tolist() == [11, 22, 11, 11] and st.scores.cpu().tolist() == [-0.5, -1.0, -1.5, -1.5]
    want = torch.full((W, TMAX), 3, dtype=torch.int32)
    want[:, 5] = torch.tensor([2, 2, 0, 1], dtype=torch.int32)
    assert torch.equal(st.anc.cpu(), want)


# =============================================================================================== 4. the reference's tokens
def small_gpt(golden):
    zz = golden("gpt_generate")
    cfgo, prefix, tk, idx = C.gpt_small(True)
    g = load_synth(mk_gpt(cfgo)).eval()
    return g, zz, torch.from_numpy(zz["start"]).cuda(), prefix[:1].cuda(), cfgo


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipGraph"])
@pytest.mark.parametrize("W", [3, 5])
def test_cached_beam_search_with_topk_equal_width_is_the_greedy_chain(golden, fp32_mode, W, use_graph):
    """topk == beam_width: the W * W candidates are W copies of the same W tokens, so the reference's generate_beam_search collapses to its
    greedy chain (verified against the reference: it returns golden gpt_generate tokens for W = 3 and 5; top-1 / top-2 gaps >= 0.044)"""
    g, zz, start, pf, _ = small_gpt(golden)
    out = g.generate_beam_search(start.clone(), 8, pf, topk=W, beam_width=W, use_cache=True, use_graph=use_graph)
    assert out.dim() == 1 and out.cpu().tolist() == zz["tokens"].tolist()
    assert g.last_beams == [zz["tokens"].tolist()] * W and len(set(g.last_beam_scores)) == 1


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipGraph"])
def test_cached_beam_search_gpt2_124m_greedy_chain(model, z, fp32_mode, use_graph):  # noqa: F811
    start, prefix = inputs_124m(z)
    out = model.generate_beam_search(start.clone(), 8, prefix, topk=5, beam_width=5, use_cache=True, use_graph=use_graph)
    assert out.cpu().tolist() == z["tokens"].tolist()


def test_cached_deterministic_beam_search_matches_reference(golden, fp32_mode):
    g, zz, start, pf, _ = small_gpt(golden)
    want = g.beam_search(start.clone(), 5, pf, beam_width=3)
    want_scores = g.last_beam_scores
    assert want == zz["beam_tokens"].tolist()
    assert g.beam_search(start.clone(), 5, pf, beam_width=3, use_cache=True) == zz["beam_tokens"].tolist()
    np.testing.assert_allclose(g.last_beam_scores, want_scores, atol=5 * 1e-4)                      # five log-probabilities, 1e-4 each


# =============================================================================================== 5. the stochastic path
W5, TOPK5, NEW5 = 4, 10, 6
# Five torch seeds picked with the float64 CPU model of oracle/ (the same search on its logits): at gpt_small's flat 211-token distribution most
# seeds meet a top-10 boundary or a pair of candidates closer than 1e-3 within six steps (114 of the first 119); these keep every decision
# at least 1.5x clear there.  The test itself measures the margins again on the forward it runs and takes the first seed that qualifies.
SEEDS5 = [2, 36, 82, 137, 162]
ORDER_MARGIN = 2e-4     # two paths' fp32 logits agree within 1e-4 (the project's logit tolerance): ranks inside the top-k can only swap below 2e-4


def host_oracle(g, start, pf, seed, temperature=1.0):
    """The re-forward beam search with the device rule: last-position logits of the un-cached forward of all beams, float64 log_softmax
    + topk, then select_ref.  -> beams (token lists), scores, and the smallest decision margin as a multiple of its threshold: 1e-3 at
    the top-k boundary, between the W-th and (W+1)-th Gumbel key and between neighbours among the W + 1 best distinct candidates
    (their order is the beam number, which keys the next draw); ORDER_MARGIN between neighbours inside the top-k (the entry number keys
    the draw too)"""
    beams, scores, margin = [start[0].cpu().tolist()] * W5, np.zeros(W5, np.float32), np.inf
    no_table = np.zeros((W5, 1), np.int32)
    for t in range(NEW5):
        with torch.no_grad():
            _, logits = g(torch.tensor(beams, device="cuda"), prefix=pf.expand(W5, -1, -1).contiguous())
        lp, ids = torch.log_softmax(logits[:, -1, :].double().cpu() / temperature, -1).topk(TOPK5 + 1, -1)
        margin = min(margin, float((lp[:, TOPK5 - 1] - lp[:, TOPK5]).min()) / 1e-3, float((lp[:, :-1] - lp[:, 1:]).min()) / ORDER_MARGIN)
        top_lp, top_id = lp[:, :TOPK5].float().numpy(), ids[:, :TOPK5].numpy()
        parent, cur, new_scores, _, key_margin, _, pick = select_ref(top_lp, top_id, t == 0, W5, scores, seed, t, -1, no_table)
        # a candidate is (history, token): one proposed twice ties exactly on both sides, distinct ones must lie apart
        drawn = sorted(((float(np.float32(scores[i] + top_lp[0 if t == 0 else i][j])), tuple(beams[i]) + (int(top_id[0 if t == 0 else i][j]),))
                        for i in range(W5) for j in pick[i]), key=lambda c: -c[0])
        gaps = [a[0] - b[0] for a, b in zip(drawn[:W5], drawn[1:W5 + 1]) if a[1] != b[1]]
        margin = min(margin, key_margin / 1e-3, (min(gaps) if gaps else np.inf) / 1e-3)
        beams, scores = [beams[p] + [c] for p, c in zip(parent, cur)], new_scores
    return beams, scores, margin


def seed_of(s):
    """the Philox seed K.BeamState draws after torch.manual_seed(s)"""
    torch.manual_seed(s)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def test_cached_stochastic_beam_search_equals_the_host_oracle(golden, fp32_mode):
    """gpt_small, W = 4, topk = 10, 6 new tokens: the cached search equals the host oracle built on the un-cached forward, beam for beam
    (token sequences; identical beams may swap places) and score for score (six log-probabilities, 1e-4 each), for the first seed of
    SEEDS5 whose decisions are all clear of the two paths' rounding"""
    g, zz, start, pf, _ = small_gpt(golden)
    for s in SEEDS5:
        want_beams, want_scores, margin = host_oracle(g, start, pf, seed_of(s))
        print(f"seed {s}: smallest decision margin {margin:.3g} x its threshold")
        if margin >= 1.0:
            break
    else:
        pytest.fail("none of the five seeds keeps every decision clear of rounding")
    for use_graph in (False, True):
        torch.manual_seed(s)
        out = g.generate_beam_search(start.clone(), NEW5, pf, topk=TOPK5, beam_width=W5, use_cache=True, use_graph=use_graph)
        assert sorted(g.last_beams) == sorted(want_beams), use_graph
        order = sorted(range(W5), key=lambda b: g.last_beams[b])
        want_order = sorted(range(W5), key=lambda b: want_beams[b])
        got_sc, want_sc = np.array(g.last_beam_scores)[order], want_scores[want_order]
        print(f"graph={use_graph}: max |score - oracle| = {float(np.abs(got_sc - want_sc).max()):.3g}")
        assert float(np.abs(got_sc - want_sc).max()) <= 6 * 1e-4
        assert out.cpu().tolist() == g.last_beams[int(np.argmax(g.last_beam_scores))]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_cached_stochastic_beam_search_graph_eager_and_seeds(golden, mode):
    g, zz, start, pf, _ = small_gpt(golden)
    fa.set_compute_dtype(mode)
    try:
        runs = {}
        for name, s, use_graph in (("eager", 21, False), ("graph", 21, True), ("again", 21, False), ("other", 22, False), ("third", 23, False)):
            torch.manual_seed(s)
            out = g.generate_beam_search(start.clone(), NEW5, pf, topk=TOPK5, beam_width=W5, use_cache=True, use_graph=use_graph)
            runs[name] = (out.cpu().tolist(), g.last_beams, g.last_beam_scores)
            assert len(out) == 4 + NEW5 and out[:4].cpu().tolist() == start[0].cpu().tolist() and max(out.cpu().tolist()) < g.config.vocab_size
            assert all(math.isfinite(x) for x in g.last_beam_scores) and len(g.last_beams) == W5
    finally:
        fa.set_compute_dtype("bf16")
    assert runs["graph"] == runs["eager"] == runs["again"]                                       # same seed: identical beams and scores
    assert runs["other"][1:] != runs["eager"][1:] or runs["third"][1:] != runs["eager"][1:]     # other seeds: other draws


# =============================================================================================== 6. fallbacks and Franky
def build_franky():
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models.notebook_models import BrainEncoder, Franky
    bcfg, gcfg, x, tok = C.cfg1()
    e = bcfg.encoder
    enc = bf.MAEConfig(window_size=e.window_size, n_electrodes=256, patch_size=25, dim=128, n_layers=2, head_dim=32,
                       hidden_dim=512, n_heads=4, n_kv_heads=4)
    cfg = bf.Config(encoder=enc, n_output_tokens=32, output_dim=128, dim=128, n_layers=2, head_dim=32, hidden_dim=256,
                    n_heads=4, n_kv_heads=4)
    fr = Franky(BrainEncoder(cfg), mk_gpt(gcfg))
    return load_synth(fr), x, gcfg


def test_franky_generate_beam(fp32_mode):
    fr, x, gcfg = build_franky()
    torch.manual_seed(3)
    out = fr.eval().generate_beam(x[0].numpy(), max_new_tokens=7)
    assert out.shape == (1 + 7,) and int(out[0]) == 50256 and int(out.max()) < gcfg.vocab_size and int(out.min()) >= 0
    assert len(fr.llm_model.last_beams) == 5 and out.cpu().tolist() in fr.llm_model.last_beams


def test_outside_the_envelope_the_re_forward_path_runs(golden, fp32_mode):
    """beam_width = 17 and a sequence one row longer than block_size (prefix 5 + prompt 4 + 56 new = 65 > 64; the re-forward loop's longest
    forward is 64 positions): use_cache=True takes the re-forward loop (which sets no last_beams) and returns a well-formed sequence"""
    g, zz, start, pf, cfgo = small_gpt(golden)
    assert cfgo.block_size == 64
    for n, kw in ((4, dict(topk=20, beam_width=17)), (56, dict(topk=6, beam_width=3))):
        g.last_beams = None
        out = g.generate_beam_search(start.clone(), n, pf, use_cache=True, **kw)
        assert g.last_beams is None
        assert out.shape == (4 + n,) and torch.equal(out[:4].cpu(), start[0].cpu()) and 0 <= int(out.min()) and int(out.max()) < cfgo.vocab_size
