"""Beam search over a batch of sentences on the MI355X: fk_attn_decode_beam_grouped and fk_beam_select_grouped against the float64 / numpy
restatements of tests/test_beam_gpu.py applied sentence by sentence, and GPT.generate_beam_search / Franky.generate_beam with S > 1
sentences against the reference's recorded tokens, the un-cached forward and the host oracle.

Layout under test: row r = g * W + b is beam b of sentence g, the caches are [S * W, Tmax, 2d], the table holds LOCAL slots in [0, W).
Every sentence gets its own random data, so a forgotten g * W reads another sentence's rows (or NaN) and is a gross error.

Tolerances are those of tests/test_beam_gpu.py: attention close() defaults in fp32 and atol 2e-2 in bf16; everything the select kernel
writes is compared exactly, where the numpy keys and scores are >= 1e-3 apart; model scores 1e-4 per log-probability."""
import math

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from tests import cases as C
from tests.test_beam_gpu import (NEW5, SEEDS5, TMAX, TOPK5, W5, K, _beam_attn_ref, build_franky, fp32_mode, grid_rows, host_oracle,  # noqa: F401
                                 i32, seed_of, select_ref, small_gpt)
from tests.test_kernels_gpu import close, dev, q, rnd

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
H = 2


# =============================================================================================== 1. fk_attn_decode_beam_grouped
def _grouped_case(S, W, D, pos, dtype, poison=True):
    """qkv [S*W, 3d], kv [S*W, TMAX, 2d], a random table of local slots; with `poison` every cache row that no entry of its own sentence
    names is NaN.  -> qkv, kv, anc (local), the same table in global slots for _beam_attn_ref"""
    R, d = S * W, H * D
    g = torch.Generator().manual_seed(100000 * S + 1000 * W + 10 * D + pos)
    qkv = q(rnd(R, 3 * d, seed=pos + 1), dtype)
    kv = q(rnd(R, TMAX, 2 * d, seed=pos + 2), dtype)
    anc = torch.randint(0, W, (R, TMAX), generator=g, dtype=torch.int32)
    base = (torch.arange(R) // W * W)[:, None]
    glob = (anc + base).to(torch.int32)
    if poison:
        used = torch.zeros(R, TMAX, dtype=torch.bool)
        used[glob[:, :pos].long().reshape(-1), torch.arange(pos).repeat(R)] = True
        used[torch.arange(R), pos] = True
        kv[~used] = float("nan")
    anc[:, pos:] = 7 * W + 3                                                                      # never read: the row pos is the beam's own
    return qkv, kv, anc, glob


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_grouped_attention_against_float64_gather_softmax(K, dtype, D):  # noqa: F811
    for S, W in ((1, 5), (3, 1), (3, 5), (2, 16)):
        for pos in (0, 1, 255, 256, 299):
            qkv, kv, anc, glob = _grouped_case(S, W, D, pos, dtype)
            got = K.attn_decode_beam_grouped(dev(qkv, dtype), dev(kv, dtype), dev(anc), i32(pos), H, S)
            assert got.shape == (S * W, H * D) and bool(torch.isfinite(got).all()), (S, W, pos)
            want = _beam_attn_ref(qkv, kv, glob, pos, H, D)
            print(f"attn_decode_beam_grouped S={S} W={W} D={D} {dtype} pos={pos}: max |o - f64| = {float((got.double().cpu() - want).abs().max()):.3g}")
            close(got, want, dtype, **({} if dtype == torch.float32 else {"atol16": 2e-2}))


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_one_group_without_append_is_attn_decode_beam_bit_for_bit(K, dtype, D):  # noqa: F811
    for pos in (0, 255, 256, 299):
        qkv, kv, anc, _ = _grouped_case(1, 5, D, pos, dtype)
        qkv, kv, anc = dev(qkv, dtype), dev(kv, dtype), dev(anc)
        got = K.attn_decode_beam_grouped(qkv, kv, anc, i32(pos), H, 1, append=False)
        assert torch.equal(got, K.attn_decode_beam(qkv, kv, anc, i32(pos), H)), pos


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_append_writes_the_new_row_and_nothing_else(K, dtype, D):  # noqa: F811
    """append=True: kv[r, pos] (NaN before) becomes qkv[r, d:] bit for bit, no other element of the cache changes, and the output is the
    one of kv_append_ followed by the launch without append"""
    S, W, d = 3, 5, H * D
    for pos in (0, 255, 256):
        qkv, kv, anc, _ = _grouped_case(S, W, D, pos, dtype, poison=False)
        kv[:, pos] = float("nan")
        qkv, kv, anc = dev(qkv, dtype), dev(kv, dtype), dev(anc)
        before = kv.clone()
        got = K.attn_decode_beam_grouped(qkv, kv, anc, i32(pos), H, S, append=True)
        assert torch.equal(_bits(kv[:, pos]), _bits(qkv[:, d:])), pos
        changed = _bits(kv) != _bits(before)
        changed[:, pos] = False
        assert not bool(changed.any()), pos
        two = before.clone()
        K.kv_append_(qkv, two, i32(pos))
        want = K.attn_decode_beam_grouped(qkv, two, anc, i32(pos), H, S, append=False)
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(want)), pos
        assert torch.equal(_bits(two), _bits(kv)), pos


@pytest.mark.parametrize("append", [False, True], ids=["read", "append"])
def test_grouped_attention_clamps_a_corrupt_table_inside_the_sentence(K, append):  # noqa: F811
    """entries anywhere in int32 read the rows the entries clamped to [0, W) name, bit for bit: never another sentence's, never outside"""
    S, W, D, pos = 3, 5, 64, 40
    qkv, kv = dev(rnd(S * W, 3 * H * D, seed=1), torch.bfloat16), dev(rnd(S * W, TMAX, 2 * H * D, seed=2), torch.bfloat16)
    anc = torch.randint(-2 ** 31, 2 ** 31 - 1, (S * W, TMAX), generator=torch.Generator().manual_seed(3), dtype=torch.int64).to(torch.int32)
    anc[:, ::3] = torch.randint(0, W, (S * W, len(range(0, TMAX, 3))), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    got = K.attn_decode_beam_grouped(qkv, kv.clone(), dev(anc), i32(pos), H, S, append=append)
    want = K.attn_decode_beam_grouped(qkv, kv.clone(), dev(anc.clamp(0, W - 1)), i32(pos), H, S, append=append)
    assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(want))


# =============================================================================================== 2. fk_beam_select_grouped
# 64 sentences x 4 beams x 3 steps are 768 draws of 4 out of 8 keys: some data puts two keys closer than 1e-3 somewhere.  These salts of the
# data generator were picked on the CPU from select_ref's own margins (the first that keeps them all >= 1e-3), before any kernel ran.
SALT = {(64, 4, 8, False): 2, (64, 4, 8, True): 1}


def _select_inputs(S, W, k, broadcast):
    """the whole input of three steps, drawn once: seeds, table, scores, and per step the top_lp / top_id rows of every sentence"""
    rng = np.random.default_rng(10000 * S + 100 * W + k + (5 if broadcast else 0) + 1000003 * SALT.get((S, W, k, broadcast), 0))
    seeds = [0x1234_5678_9ABC_DEF0 + 977 * g + W for g in range(S)]
    anc = rng.integers(0, W, (S * W, TMAX)).astype(np.int32)
    scores = np.concatenate([grid_rows(rng, 1, W)[0] for _ in range(S)])
    rows = S if broadcast else S * W
    steps = [(grid_rows(rng, rows, k), np.stack([rng.choice(50257, k, replace=False) for _ in range(rows)]).astype(np.int64)) for _ in range(3)]
    return seeds, anc, scores, steps


@pytest.mark.parametrize("broadcast", [False, True], ids=["row_stride=k", "row_stride=0"])
@pytest.mark.parametrize("S,W,k", [(1, 4, 20), (3, 4, 20), (3, 16, 16), (8, 1, 1), (64, 4, 8)])
def test_beam_select_grouped_three_steps_against_numpy(K, S, W, k, broadcast):  # noqa: F811
    """three consecutive steps on one state from *pos = 254, select_ref applied to every sentence with that sentence's seed: tokens,
    scores, both logs, the whole table, exact; after every launch the ticket is back at zero and the ONE step counter and the ONE position
    have advanced by exactly one (S blocks that each incremented would show here); the third step finds no log row and writes none.  With
    S = 1 the state also equals the one K.beam_select leaves from the same start."""
    seeds, anc, scores, steps = _select_inputs(S, W, k, broadcast)
    pos0, log_rows = 254, 2
    st = K.BeamState("cuda", W, log_rows, TMAX, seed=seeds, groups=S)
    plog = torch.full((3, S * W), -5, dtype=torch.int32, device="cuda")                            # one row more than the state announces
    tlog = torch.full((3, S * W), -5, dtype=torch.int64, device="cuda")
    st.parent_log, st.tok_log = plog[:log_rows], tlog[:log_rows]
    st.anc.copy_(torch.from_numpy(anc))
    st.scores.copy_(torch.from_numpy(scores))
    cur, pos = torch.empty(S * W, dtype=torch.int64, device="cuda"), i32(pos0)
    if S == 1:
        one = K.BeamState("cuda", W, log_rows, TMAX, seed=seeds[0])
        one.anc.copy_(st.anc)
        one.scores.copy_(st.scores)
        one.parent_log.fill_(-5)
        one.tok_log.fill_(-5)
        one_cur, one_pos = torch.empty(W, dtype=torch.int64, device="cuda"), i32(pos0)
    for t, (top_lp, top_id) in enumerate(steps):
        want_parent, want_cur = [], []
        for g in range(S):
            rows = slice(g, g + 1) if broadcast else slice(g * W, g * W + W)
            sl = slice(g * W, g * W + W)
            parent, c, scores[sl], anc[sl], key_margin, score_margin, _ = select_ref(top_lp[rows], top_id[rows], broadcast, W, scores[sl], seeds[g], t,
                                                                                     pos0 + t, anc[sl])
            assert key_margin >= 1e-3 and score_margin >= 1e-3, (g, t, key_margin, score_margin)
            want_parent += parent
            want_cur += c
        lp_d, id_d = dev(torch.from_numpy(top_lp)), dev(torch.from_numpy(top_id))
        K.beam_select_grouped(lp_d, id_d, st, cur, pos, pos_inc=pos, broadcast=broadcast)
        assert int(st.ticket) == 0 and int(st.step) == t + 1 and int(pos) == pos0 + t + 1, t
        assert cur.cpu().tolist() == want_cur, t
        assert np.array_equal(st.scores.cpu().numpy(), scores), t
        assert np.array_equal(st.anc.cpu().numpy(), anc), t
        if t < log_rows:
            assert plog[t].cpu().tolist() == want_parent and tlog[t].cpu().tolist() == want_cur, t
        if S == 1:
            K.beam_select(lp_d, id_d, one, one_cur, one_pos, pos_inc=one_pos, broadcast=broadcast)
            assert torch.equal(one_cur, cur) and torch.equal(one.scores, st.scores) and torch.equal(one.anc, st.anc), t
            assert torch.equal(one.parent_log, st.parent_log) and torch.equal(one.tok_log, st.tok_log), t
            assert int(one.step) == int(st.step) and int(one_pos) == int(pos), t
    assert bool((plog[log_rows:] == -5).all()) and bool((tlog[log_rows:] == -5).all())             # the third step wrote no log row


# =============================================================================================== 3. the model: greedy collapse
def three_sentences():
    cfgo, prefix, tk, idx = C.gpt_small(True)
    return idx[:3, :4].contiguous().cuda(), prefix[:3].contiguous().cuda()


_chains = {}


def greedy_chains(g, starts, pf):
    """argmax chain of the un-cached forward for every sentence (8 tokens), computed once; asserts its own top-1 / top-2 gap >= 1e-3 at
    every step, so the cached fp32 step (logits within 1e-4) cannot pick another token"""
    if "c" not in _chains:
        seq = starts.clone()
        for _ in range(8):
            with torch.no_grad():
                _, logits = g(seq, prefix=pf)
            top2 = logits[:, -1, :].float().topk(2, -1)
            gap = float((top2.values[:, 0] - top2.values[:, 1]).min())
            assert gap >= 1e-3, gap
            seq = torch.cat((seq, top2.indices[:, :1]), 1)
        _chains["c"] = seq.cpu().tolist()
    return _chains["c"]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipGraph"])
@pytest.mark.parametrize("W", [3, 5])
def test_batched_search_with_topk_equal_width_is_every_sentence_s_greedy_chain(golden, fp32_mode, W, use_graph):  # noqa: F811
    g, zz, start, _, _ = small_gpt(golden)
    starts, pf = three_sentences()
    assert torch.equal(starts[:1], start)
    chains = greedy_chains(g, starts, pf)
    assert chains[0] == zz["tokens"].tolist()
    out = g.generate_beam_search(starts.clone(), 8, pf, topk=W, beam_width=W, use_cache=True, use_graph=use_graph)
    assert out.shape == (3, 12) and out.cpu().tolist() == chains
    assert g.last_beams == [[c] * W for c in chains]
    assert len(g.last_beam_scores) == 3 and all(len(s) == W and len(set(s)) == 1 for s in g.last_beam_scores)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipGraph"])
def test_batched_search_of_twenty_rows_takes_the_gemm_route_to_the_same_chains(golden, fp32_mode, use_graph):  # noqa: F811
    """S = 4 (sentences 0, 1, 2, 0) x W = 5 = 20 rows: past the 16 rows of the weight-streaming step, the linear layers are MFMA GEMMs"""
    g, zz, _, _, _ = small_gpt(golden)
    starts, pf = three_sentences()
    chains = greedy_chains(g, starts, pf)
    sel = [0, 1, 2, 0]
    out = g.generate_beam_search(starts[sel].contiguous(), 8, pf[sel].contiguous(), topk=5, beam_width=5, use_cache=True, use_graph=use_graph)
    assert out.shape == (4, 12) and out.cpu().tolist() == [chains[s] for s in sel]
    assert g.last_beams == [[chains[s]] * 5 for s in sel]


# =============================================================================================== 4. the model: stochastic
# Philox seeds per sentence, picked with the float64 CPU model of oracle/ (the host oracle's search on its logits) so that every decision
# stays >= 1.5x clear of its threshold there.  Sentence 0: the seeds K.BeamState draws after torch.manual_seed(s), s in SEEDS5.
CANDIDATES = [
    None,
    [1000003, 1000005, 1000007, 1000008, 1000009, 1000011],
    [2000006, 2000007, 2000010, 2000012, 2000013, 2000014],
]


def test_batched_stochastic_search_equals_the_host_oracle_sentence_by_sentence(golden, fp32_mode):  # noqa: F811
    """gpt_small, W = 4, topk = 10, 6 new tokens, three sentences with explicit seeds: every sentence of the batched search equals the host
    oracle of that sentence alone with its seed (beams as a set, scores within six log-probabilities of 1e-4, the returned row its best
    beam), eager and as a hipGraph"""
    g, zz, _, _, _ = small_gpt(golden)
    starts, pf = three_sentences()
    seeds, want = [], []
    for s in range(3):
        for cand in ([seed_of(x) for x in SEEDS5] if s == 0 else CANDIDATES[s]):
            beams, scores, margin = host_oracle(g, starts[s:s + 1], pf[s:s + 1], cand)
            print(f"sentence {s} seed {cand}: smallest decision margin {margin:.3g} x its threshold")
            if margin >= 1.0:
                break
        else:
            pytest.fail(f"none of sentence {s}'s candidate seeds keeps every decision clear of rounding")
        seeds.append(cand)
        want.append((beams, scores))
    for use_graph in (False, True):
        out = g.generate_beam_search(starts.clone(), NEW5, pf, topk=TOPK5, beam_width=W5, use_cache=True, use_graph=use_graph, seeds=seeds)
        assert out.shape == (3, 4 + NEW5)
        for s, (want_beams, want_scores) in enumerate(want):
            got_beams, got_scores = g.last_beams[s], g.last_beam_scores[s]
            assert sorted(got_beams) == sorted(want_beams), (s, use_graph)
            order = sorted(range(W5), key=lambda b: got_beams[b])
            want_order = sorted(range(W5), key=lambda b: want_beams[b])
            err = float(np.abs(np.array(got_scores)[order] - want_scores[want_order]).max())
            print(f"sentence {s} graph={use_graph}: max |score - oracle| = {err:.3g}")
            assert err <= 6 * 1e-4
            assert out[s].cpu().tolist() == got_beams[int(np.argmax(got_scores))]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_batched_stochastic_search_seeds_make_a_sentence_reproducible_on_its_own(golden, mode):
    g, zz, _, _, _ = small_gpt(golden)
    starts, pf = three_sentences()
    fa.set_compute_dtype(mode)
    try:
        runs = {}
        for name, seeds, use_graph in (("eager", [11, 12, 13], False), ("graph", [11, 12, 13], True), ("again", [11, 12, 13], False),
                                       ("other", [11, 99, 13], False), ("third", [11, 98, 13], False)):
            out = g.generate_beam_search(starts.clone(), NEW5, pf, topk=TOPK5, beam_width=W5, use_cache=True, use_graph=use_graph, seeds=seeds)
            runs[name] = (out.cpu().tolist(), g.last_beams, g.last_beam_scores)
            assert out.shape == (3, 4 + NEW5) and torch.equal(out[:, :4], starts) and int(out.max()) < g.config.vocab_size and int(out.min()) >= 0
            assert all(math.isfinite(x) for s in g.last_beam_scores for x in s) and [len(b) for b in g.last_beams] == [W5] * 3
    finally:
        fa.set_compute_dtype("bf16")
    assert runs["graph"] == runs["eager"] == runs["again"]                                       # same seeds: identical beams and scores
    for name in ("other", "third"):                                                              # only seeds[1] changed: sentences 0 and 2 stay
        for s in (0, 2):
            assert [part[s] for part in runs[name]] == [part[s] for part in runs["eager"]], (name, s)
    assert any([part[1] for part in runs[name][1:]] != [part[1] for part in runs["eager"][1:]] for name in ("other", "third"))


# =============================================================================================== 5. envelope and Franky
def test_two_sentences_outside_the_envelope_take_the_re_forward_loop(golden, fp32_mode):  # noqa: F811
    """beam_width = 17, and a sequence one row longer than block_size (5 + 4 + 56 = 65 > 64): S = 2 runs the re-forward loop once per
    sentence (which sets no last_beams) and returns well-formed rows"""
    g, zz, _, _, cfgo = small_gpt(golden)
    starts, pf = three_sentences()
    assert cfgo.block_size == 64
    for n, kw in ((4, dict(topk=20, beam_width=17)), (56, dict(topk=6, beam_width=3))):
        g.last_beams = None
        out = g.generate_beam_search(starts[:2].clone(), n, pf[:2], use_cache=True, **kw)
        assert g.last_beams is None
        assert out.shape == (2, 4 + n) and torch.equal(out[:, :4], starts[:2]) and 0 <= int(out.min()) and int(out.max()) < cfgo.vocab_size


def test_franky_generate_beam_over_a_batch_of_trials(fp32_mode):  # noqa: F811
    fr, x, gcfg = build_franky()
    fr.eval()
    torch.manual_seed(3)
    for kw in ({}, {"batch_sentences": 2}):                                                       # one chunk of 3; chunks of 2 + 1
        out = fr.generate_beam(x[:3].numpy(), max_new_tokens=7, **kw)
        assert out.shape == (3, 8) and bool((out[:, 0] == 50256).all()) and int(out.max()) < gcfg.vocab_size and int(out.min()) >= 0
    one = fr.generate_beam(x[0].numpy(), max_new_tokens=7)
    assert one.shape == (8,) and int(one[0]) == 50256 and len(fr.llm_model.last_beams) == 5 and one.cpu().tolist() in fr.llm_model.last_beams
