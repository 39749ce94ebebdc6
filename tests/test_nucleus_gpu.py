"""Nucleus (top-p) sampling on the MI355X: fk_sample_topp against the float64 restatement of its rule (tests/test_nucleus_cpu.py nucleus_ref),
against fk_sample_topk at top_p = 1 and against itself in its end-of-text mode, and GPT.generate / Franky.generate with top_p on every path.

Kernel level: one launch over ROWS identical rows gives ROWS independent draws (the Philox counter holds the row), LAUNCHES launches of one
state ROWS * LAUNCHES.  Every case compared with the restatement first asserts a margin >= 0.02 between every token's mass_gt / total and
top_p (the header lets a token within 1e-4 of the boundary fall on either side), then:
  no draw falls outside the kept set, every kept head token is drawn, and for at most six kept tokens the total variation against the exact
  renormalised distribution is below 2.5 * sqrt(m / (2 pi n)) (m kept tokens, n draws: the square root is the expected sampling noise,
  2.5 the factor tests/test_kernels_gpu.py test_sample_topk_on_device allows over it, 0.03 against 0.0126)."""
import math

import numpy as np
import pytest
import torch

import frankenstein_amd as fa  # noqa: F401
from tests.test_beam_gpu import K, build_franky, fp32_mode, i32, small_gpt  # noqa: F401
from tests.test_kernels_gpu import rnd
from tests.test_nucleus_cpu import CASES, HEADS, MIN_MARGIN, POS_1000, crafted_row, nucleus_ref

pytestmark = pytest.mark.gpu

ROWS, LAUNCHES = 2048, 10
POS_GPT2 = (1024, 0, 50256, 49, 1023, 50)     # the first index, both sides of thread 0's chunk boundary (50 per thread), a multiple of the block size, the last


def identical_rows(row, rows, stride):
    """[rows, V] view with row stride `stride` >= V of `rows` copies of the fp32 row; the columns behind V hold defined values (zeros)"""
    wide = torch.zeros(rows, stride)
    wide[:, :row.size] = torch.from_numpy(row)
    return wide.cuda()[:, :row.size]


def draw(K, logits, T, top_k, top_p, launches, seed=2024):  # noqa: F811
    """-> int64 [rows * launches] on the host; checks the counters"""
    state = K.SampleState("cuda", seed=seed)
    out = torch.full((logits.shape[0], launches), -1, dtype=torch.int64, device="cuda")
    pos = i32(3)
    for _ in range(launches):
        K.sample_topp(logits, T, top_k, top_p, state, out=out, pos_inc=pos)
    assert int(state.step) == launches and int(pos) == 3 + launches and int(state.ticket) == 0
    return out.cpu().numpy().reshape(-1)


def check_membership(tok, kept, head_pos, V):
    cnt = np.bincount(tok, minlength=V)
    assert tok.min() >= 0 and tok.max() < V
    assert int(cnt[~kept].sum()) == 0, np.nonzero(cnt * ~kept)[0][:8]
    assert all(cnt[i] > 0 for i in head_pos if kept[i]), [int(cnt[i]) for i in head_pos]
    return cnt


def check_distribution(cnt, kept, probs, n):
    m = int(kept.sum())
    tv = 0.5 * float(np.abs(cnt / n - probs).sum())
    bound = 2.5 * math.sqrt(m / (2 * math.pi * n))
    print(f"kept {m}, n {n}: total variation {tv:.5f} (bound {bound:.5f})")
    assert tv < bound, (tv, bound)


# =============================================================================================== 1. the crafted row, V = 1000
@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("case", sorted(CASES, key=str), ids=lambda c: f"p{c[0]}-k{c[1]}")
def test_sample_topp_draws_the_nucleus_of_the_crafted_row(K, case, T):  # noqa: F811
    top_p, top_k = case
    heads, tail = CASES[case]
    row = crafted_row(1000, POS_1000, T)
    kept, margin, probs = nucleus_ref(row, T, top_k, top_p)
    assert margin >= MIN_MARGIN, margin
    assert int(kept.sum()) == heads + (994 if tail else 0)
    tok = draw(K, identical_rows(row, ROWS, 1024), T, top_k, top_p, LAUNCHES)
    n = ROWS * LAUNCHES
    cnt = check_membership(tok, kept, POS_1000, 1000)
    if int(kept.sum()) <= 6:
        check_distribution(cnt, kept, probs, n)
    if tail:                                                             # (.92, -): the 994 equal logits all stay and hold .11 together
        share = 1.0 - cnt[list(POS_1000)].sum() / n
        print(f"tail share {share:.5f}")
        assert abs(share - 0.11) <= 5 * math.sqrt(0.11 * 0.89 / n), share


def test_sample_topp_across_the_sign_of_the_keys(K):  # noqa: F811
    """the crafted row shifted by +5: the heads are positive, the tail is negative, and at .92 the nucleus reaches across"""
    T, top_p = 0.7, 0.92
    row = crafted_row(1000, POS_1000, T, shift=5.0)
    assert (row[list(POS_1000)] > 0).all() and int((row < 0).sum()) == 994
    kept, margin, probs = nucleus_ref(row, T, None, top_p)
    assert margin >= MIN_MARGIN and bool(kept.all())
    tok = draw(K, identical_rows(row, ROWS, 1024), T, None, top_p, LAUNCHES)
    cnt = check_membership(tok, kept, POS_1000, 1000)
    share = 1.0 - cnt[list(POS_1000)].sum() / tok.size
    assert abs(share - 0.11) <= 5 * math.sqrt(0.11 * 0.89 / tok.size), share


@pytest.mark.parametrize("top_p,count", [(0.10, 1), (0.42, 3), (0.75, 5)])
def test_sample_topp_when_the_last_radix_pass_decides(K, top_p, count):  # noqa: F811
    """six logits 1 + i * 2^-20: their keys differ in the lowest byte only and each holds a sixth of the mass; the rest are -30"""
    pos = (5, 900, 64, 63, 999, 400)
    row = np.full(1000, -30.0, np.float32)
    row[list(pos)] = [np.float32(1.0 + i * 2.0 ** -20) for i in range(6)]
    keys = row[list(pos)].view(np.uint32)
    assert len(set(keys >> 8)) == 1 and len(set(keys & 255)) == 6
    kept, margin, probs = nucleus_ref(row, 1.0, None, top_p)
    assert margin >= MIN_MARGIN, margin
    assert int(kept.sum()) == count and [bool(kept[i]) for i in pos] == [i >= 6 - count for i in range(6)]
    tok = draw(K, identical_rows(row, ROWS, 1024), 1.0, None, top_p, 2)
    cnt = check_membership(tok, kept, pos, 1000)
    assert int((cnt > 0).sum()) == count
    check_distribution(cnt, kept, probs, tok.size)


def test_sample_topp_with_negative_keys_and_a_masked_entry(K):  # noqa: F811
    """the crafted row shifted by -5 and its .06 head at -inf: at .60 of the remaining .94 the first three heads stay"""
    T, top_p = 0.7, 0.60
    row = crafted_row(1000, POS_1000, T, shift=-5.0)
    row[POS_1000[5]] = -np.inf
    assert (row < 0).all()
    kept, margin, probs = nucleus_ref(row, T, None, top_p)
    assert margin >= MIN_MARGIN, margin
    assert int(kept.sum()) == 3 and all(kept[i] for i in POS_1000[:3])
    tok = draw(K, identical_rows(row, ROWS, 1024), T, None, top_p, LAUNCHES)
    cnt = check_membership(tok, kept, POS_1000, 1000)
    assert cnt[POS_1000[5]] == 0
    check_distribution(cnt, kept, probs, tok.size)


# =============================================================================================== 2. the GPT-2 vocabulary
@pytest.mark.parametrize("case", [(0.70, None), (0.70, 5)], ids=lambda c: f"p{c[0]}-k{c[1]}")
def test_sample_topp_on_the_gpt2_vocabulary(K, case):  # noqa: F811
    top_p, top_k = case
    V, B, T = 50257, 64, 0.7
    row = crafted_row(V, POS_GPT2, T)
    kept, margin, probs = nucleus_ref(row, T, top_k, top_p)
    assert margin >= MIN_MARGIN, margin
    assert int(kept.sum()) == CASES[case][0] and kept[50256] and kept[0]
    tok = draw(K, identical_rows(row, B, V), T, top_k, top_p, LAUNCHES)
    check_membership(tok, kept, POS_GPT2, V)


# =============================================================================================== 3. top_p = 1, seeds, counters
@pytest.mark.parametrize("top_k", [None, 40])
def test_sample_topp_at_one_equals_sample_topk(K, top_k):  # noqa: F811
    """the Philox counter layout is unchanged and at top_p = 1 nothing is cropped: token for token over 50 steps.  (No restatement here, so
    no margin: the lowest token's mass_gt / total is always within its own probability of 1.)"""
    T = 0.8
    lg = (rnd(3, 1024, seed=3) * 2.0).cuda()[:, :1000]
    wide = (rnd(1, 50257, seed=4) * 3.0).cuda()
    for logits in (lg, wide):
        B = logits.shape[0]
        a, b = K.SampleState("cuda", seed=77), K.SampleState("cuda", seed=77)
        out_a, out_b = (torch.full((B, 50), -1, dtype=torch.int64, device="cuda") for _ in range(2))
        for _ in range(50):
            K.sample_topk(logits, T, top_k, a, out=out_a)
            K.sample_topp(logits, T, top_k, 1.0, b, out=out_b)
        assert torch.equal(out_a, out_b)
        assert int(b.step) == 50 and int(b.ticket) == 0


def test_sample_topp_is_reproducible_from_the_seed_and_advances_once_per_launch(K):  # noqa: F811
    T, top_p = 0.7, 0.70
    rows = np.stack([crafted_row(1000, POS_1000[b:] + POS_1000[:b], T) for b in range(5)])            # the heads rotate through the positions
    for r in rows:
        assert nucleus_ref(r, T, None, top_p)[1] >= MIN_MARGIN
    logits = torch.from_numpy(rows).cuda()
    runs = []
    for seed in (5, 5, 6):
        st = K.SampleState("cuda", seed=seed, step=2)
        pos = i32(9)
        out = torch.full((5, 8), -7, dtype=torch.int64, device="cuda")
        cur = torch.empty(5, dtype=torch.int64, device="cuda")
        for t in range(4):
            got = K.sample_topp(logits, T, None, top_p, st, cur=cur, out=out, pos_inc=pos)
            assert got is cur and int(st.step) == 3 + t and int(pos) == 10 + t and int(st.ticket) == 0
            assert torch.equal(out[:, 2 + t], cur)
        assert bool((out[:, :2] == -7).all()) and bool((out[:, 6:] == -7).all())
        runs.append(out.cpu())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    # a step counter past the buffer is not a write past it
    small = out[:, :3]
    for _ in range(2):
        K.sample_topp(logits, T, None, top_p, st, out=small)
    assert int(st.step) == 8 and torch.equal(out.cpu(), runs[2])


# =============================================================================================== 4. the end-of-text mode
def test_sample_topp_end_of_text_mode(K):  # noqa: F811
    """six rows of the crafted row with the heads rotated through six positions, top_p = .70 (the first four heads stay), 12 steps; the id is
    the position that holds the .20 / .30 / .06 / .08 / .10 / .15 head of rows 0 .. 5, so rows 2 and 3 can never draw it.  Row 5 starts done.
    Every row's tokens up to its first id are the plain-mode call's with the same seed; behind it the row emits the id and draws nothing."""
    T, top_p, S, B = 0.7, 0.70, 12, 6
    spots = (7, 130, 131, 500, 640, 999)
    eos = spots[1]
    rows = np.stack([crafted_row(1000, [spots[(j + b) % 6] for j in range(6)], T) for b in range(B)])
    head_at_eos = [HEADS[(1 - b) % 6] for b in range(B)]
    assert head_at_eos == [0.20, 0.30, 0.06, 0.08, 0.10, 0.15]
    for b, r in enumerate(rows):
        kept, margin, _ = nucleus_ref(r, T, None, top_p)
        assert margin >= MIN_MARGIN and int(kept.sum()) == 4 and bool(kept[eos]) == (head_at_eos[b] >= 0.10)
    logits = torch.from_numpy(rows).cuda()
    a, b_ = K.SampleState("cuda", seed=31), K.SampleState("cuda", seed=31)
    es = K.SampleEosState("cuda", B, eos)
    es.done[5] = 1
    es.len[5] = 4
    out_a, out_b = (torch.full((B, S), -9, dtype=torch.int64, device="cuda") for _ in range(2))
    pos = i32(10)
    lives = []
    for t in range(S):
        K.sample_topp(logits, T, None, top_p, a, out=out_a)
        cur = K.sample_topp(logits, T, None, top_p, b_, es, out=out_b, pos_inc=pos)
        assert torch.equal(cur, out_b[:, t])
        lives.append(int(es.live))
    assert int(b_.step) == S and int(b_.ticket) == 0 and int(es.live_acc) == 0 and int(pos) == 10 + S
    plain, got = out_a.cpu().numpy(), out_b.cpu().numpy()
    first = [next((t for t in range(S) if plain[r, t] == eos), None) for r in range(B)]
    assert first[2] is None and first[3] is None and any(f is not None and 0 < f < S - 1 for f in first[:2] + first[4:5]), first
    want_len, want_done = [], []
    for r in range(5):
        f = first[r]
        assert got[r].tolist() == plain[r, :S if f is None else f + 1].tolist() + [eos] * (0 if f is None else S - f - 1), r
        want_len.append(S if f is None else f + 1)
        want_done.append(0 if f is None else 1)
    assert got[5].tolist() == [eos] * S
    assert es.len.cpu().tolist() == want_len + [4] and es.done.cpu().tolist() == want_done + [1]
    for t in range(S):
        assert lives[t] == sum(1 for r in range(5) if first[r] is None or first[r] > t), t
    # eos = -1: nothing ever finishes, and a set done flag is not read
    none = K.SampleEosState("cuda", B, None)
    none.done[0] = 1
    c = K.SampleState("cuda", seed=31)
    assert K.sample_topp(logits, T, None, top_p, c, none).cpu().tolist() == plain[:, 0].tolist() and int(none.live) == B


# =============================================================================================== 5. GPT.generate and Franky.generate
NEW = 12
TINY = 1e-6          # the most likely token holds more than this: it stays alone, and generate must return the tokens of top_k = 1

PATHS = {"re-forward": dict(use_cache=False), "cached eager": dict(use_cache=True, use_graph=False), "hipGraph": dict(use_cache=True, use_graph=True)}


@pytest.fixture(scope="module")
def greedy(golden):
    g, _, start, pf, _ = small_gpt(golden)
    return g, start, pf, None


@pytest.mark.parametrize("path", sorted(PATHS))
def test_generate_with_a_tiny_top_p_is_greedy_on_every_path(greedy, fp32_mode, path):  # noqa: F811
    g, start, pf, _ = greedy
    want = g.generate(start.clone(), NEW, prefix=pf, top_k=1, **PATHS[path]).cpu().tolist()
    assert len(want) == 4 + NEW
    for top_k in (None, 10):
        torch.manual_seed(1)
        assert g.generate(start.clone(), NEW, prefix=pf, top_k=top_k, top_p=TINY, **PATHS[path]).cpu().tolist() == want, top_k


@pytest.mark.parametrize("path", sorted(PATHS))
def test_generate_with_a_tiny_top_p_and_an_end_of_text_id_is_greedy_on_every_path(greedy, fp32_mode, path):  # noqa: F811
    g, start, pf, _ = greedy
    chain = g.generate(start.clone(), NEW, prefix=pf, top_k=1, **PATHS[path]).cpu().tolist()
    gen = chain[4:]
    j = next((j for j in range(2, NEW - 1) if gen[j] not in gen[:j]), NEW - 1)          # the id: a token the greedy chain first emits inside the call
    eos = gen[j]
    want = g.generate(start.clone(), NEW, prefix=pf, top_k=1, eos_token_id=eos, check_every=2, **PATHS[path]).cpu().tolist()
    want_len, want_tokens = g.last_lengths.cpu().tolist(), g.last_tokens.cpu().tolist()
    assert want == chain[:4 + j + 1] + [eos] * (NEW - j - 1) and want_len == [j + 1]
    torch.manual_seed(1)
    got = g.generate(start.clone(), NEW, prefix=pf, top_p=TINY, eos_token_id=eos, check_every=2, **PATHS[path]).cpu().tolist()
    assert got == want and g.last_lengths.cpu().tolist() == want_len and g.last_tokens.cpu().tolist() == want_tokens


def test_generate_top_p_none_and_one_draw_what_the_call_without_it_draws(greedy, fp32_mode):  # noqa: F811
    g, start, pf, _ = greedy
    for path in ("cached eager", "hipGraph"):
        runs = []
        for kw in ({}, dict(top_p=None), dict(top_p=1.0), dict(top_p=0.5)):
            torch.manual_seed(7)
            runs.append(g.generate(start.clone(), NEW, prefix=pf, top_k=20, **kw, **PATHS[path]).cpu().tolist())
        assert runs[0] == runs[1] == runs[2], path
        assert runs[3] != runs[0], path          # 12 draws from gpt_small's flat top-20 against the top half of their mass


@pytest.fixture(scope="module")
def franky():
    fr, x, gcfg = build_franky()
    return fr.eval(), x, gcfg


def test_franky_generate_passes_top_p_on(franky, fp32_mode):  # noqa: F811
    fr, x, gcfg = franky
    want = fr.generate(x[0].numpy(), max_new_tokens=NEW, top_k=1).cpu().tolist()
    torch.manual_seed(2)
    assert fr.generate(x[0].numpy(), max_new_tokens=NEW, top_p=TINY).cpu().tolist() == want
    want = fr.generate(x[0].numpy(), max_new_tokens=NEW, top_k=1, stop=True).cpu().tolist()
    want_len = fr.last_lengths.tolist()
    torch.manual_seed(2)
    assert fr.generate(x[0].numpy(), max_new_tokens=NEW, top_p=TINY, stop=True).cpu().tolist() == want and fr.last_lengths.tolist() == want_len


def test_generate_with_top_p_as_a_graph_stays_inside_the_vocabulary(franky, fp32_mode):  # noqa: F811
    """70 new tokens of the 50 257-token decoder of the Franky configuration, top_p = .9 without a top-k crop, captured and replayed"""
    fr, x, gcfg = franky
    g = fr.llm_model
    start = torch.full((2, 1), 50256, dtype=torch.long, device="cuda")
    torch.manual_seed(4)
    out = g.generate(start, 70, top_p=0.9, use_graph=True)
    assert out.shape == (71,) and int(out.min()) >= 0 and int(out.max()) < gcfg.vocab_size
    torch.manual_seed(4)
    assert torch.equal(g.generate(start, 70, top_p=0.9, use_graph=True), out)
