"""End-of-text aware decoding on the MI355X: fk_beam_select_eos, fk_beam_backtrack and fk_sample_topk_eos against numpy restatements and
against the kernels they extend, and GPT.generate / GPT.generate_beam_search / Franky with an end-of-text id against the reference's
recorded tokens, the host oracle of tests/test_beam_gpu.py extended by the rules, and each other.

Everything the select step writes is compared exactly: raw scores are single fp32 additions, the normalised rank key is one fp32
multiply behind it on both sides, and Gumbel keys are only compared where they lie >= 1e-3 apart (asserted)."""
import numpy as np
import pytest
import torch

import frankenstein_amd as fa  # noqa: F401
from tests.test_beam_batched_gpu import three_sentences
from tests.test_beam_gpu import (NEW5, ORDER_MARGIN, TMAX, TOPK5, W5, K, build_franky, fp32_mode, grid_rows, i32, philox4x32_10,  # noqa: F401
                                 seed_of, select_ref, small_gpt)
from tests.test_decode_gpt2_gpu import inputs as inputs_124m
from tests.test_decode_gpt2_gpu import model, z  # noqa: F401  (module-scoped fixtures: GPT-2 124M and its golden file)
from tests.test_decode_loop_cpu import CASES as LOOP_CASES
from tests.test_decode_loop_cpu import expected_steps, run_counted
from tests.test_eos_cpu import eos_step_ref, lenpow_table
from tests.test_kernels_gpu import dev, rnd

pytestmark = pytest.mark.gpu

ALPHAS = [0.0, 1.0, 0.6]
BASE, EOS = 1000, 1007            # the select tests draw their ids from BASE .. BASE + 39


def gumbel_draws(top_lp, broadcast, W, seed, step):
    """the draws of fk_beam_select (tests/test_beam_gpu.py select_ref): picks[i] = beam i's entries by draw rank, margins[i] = the gap
    between its W-th and (W+1)-th Gumbel key (inf when k == W)"""
    f32 = np.float32
    k = top_lp.shape[1]
    picks, margins = [], []
    for i in range(W):
        row = top_lp[0 if broadcast else i]
        keys = np.empty(k, f32)
        for j in range(k):
            c0 = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (step & 0xFFFFFFFF, step >> 32, i, 0xBEA30000 | j))[0]
            u = (f32(c0 >> 8) + f32(0.5)) * f32(1.0 / 16777216.0)
            keys[j] = row[j] - np.log(-np.log(u, dtype=f32), dtype=f32)
        order = sorted(range(k), key=lambda j: (-keys[j], j))
        margins.append(float(keys[order[W - 1]] - keys[order[W]]) if k > W else np.inf)
        picks.append(order[:W])
    return picks, margins


def table_update(anc, parent, pos):
    new = anc.copy()
    if pos >= 0:
        W = anc.shape[0]
        old = anc[:, :pos + 1].copy()
        old[:, pos] = np.arange(W)
        new[:, :pos + 1] = old[parent]
    return new


def eos_state(K, S, W, log_rows, seeds, eos, table):
    st = K.BeamState("cuda", W, log_rows, TMAX, seed=seeds, groups=S, eos=0 if eos is None else eos)
    st.eos, st.inv_lenpow = eos, dev(torch.from_numpy(table))                                       # eos = None: the kernel gets -1
    return st


# =============================================================================================== 1. fk_beam_select_eos against numpy
# Salts of the data generator, picked on the CPU from the margins of the restatement itself (the first that keeps every Gumbel-key margin
# of a live beam >= 1e-3), before any kernel ran.
SALT = {(1, 4, 20, 0.0): 8, (1, 4, 20, 0.6): 7, (3, 4, 20, 0.0): 4, (3, 4, 20, 1.0): 2, (3, 4, 20, 0.6): 4, (2, 16, 16, 1.0): 2, (2, 16, 20, 0.0): 1,
        (2, 16, 20, 1.0): 2}
SHAPES = [(1, 1, 1), (1, 4, 20), (3, 4, 20), (2, 16, 16), (2, 16, 20)]
N_TABLE = 6                      # lengths start at 0 .. 4 and grow by three: the longest beams index past the table (clamped)


def _fin_pattern(S, W, g, rng):
    """S = 3: all finished / none / mixed; S = 2: mixed / all; S = 1: mixed (W = 1: none)"""
    kind = {3: ["all", "none", "mixed"], 2: ["mixed", "all"], 1: ["mixed" if W > 1 else "none"]}[S][g]
    if kind == "mixed":
        f = rng.integers(0, 2, W)
        f[0], f[W - 1] = 1, 0
        return f.astype(np.int32)
    return np.full(W, 1 if kind == "all" else 0, np.int32)


def eos_three_steps(S, W, k, alpha, broadcast=False):
    """the inputs of three steps and everything the restatement expects behind each -> (init, steps, smallest live key margin)"""
    rng = np.random.default_rng(10000 * S + 100 * W + k + 1000003 * SALT.get((S, W, k, alpha), 0) + int(alpha * 10))
    seeds = [0x1234_5678_9ABC_DEF0 + 977 * g + W for g in range(S)]
    table = lenpow_table(N_TABLE, alpha)
    anc = rng.integers(0, W, (S * W, TMAX)).astype(np.int32)
    scores = np.concatenate([grid_rows(rng, 1, W)[0] for _ in range(S)])
    lens = rng.integers(0, 5, S * W).astype(np.int32)
    fin = np.concatenate([_fin_pattern(S, W, g, rng) for g in range(S)])
    init = dict(seeds=seeds, table=table, anc=anc.copy(), scores=scores.copy(), lens=lens.copy(), fin=fin.copy())
    rows = S if broadcast else S * W
    pos0, steps, margin = 254, [], np.inf
    for t in range(3):
        top_lp = grid_rows(rng, rows, k)
        top_id = np.stack([BASE + rng.choice(40, k, replace=False) for _ in range(rows)]).astype(np.int64)
        parent, cur, live, newly = [], [], 0, 0
        for g in range(S):
            sl = slice(g * W, g * W + W)
            r = slice(g, g + 1) if broadcast else sl
            picks, margins = gumbel_draws(top_lp[r], broadcast, W, seeds[g], t)
            margin = min([margin] + [m for m, f in zip(margins, fin[sl]) if not f])
            p, c, scores[sl], lens[sl], f, _ = eos_step_ref(top_lp[r], top_id[r], broadcast, W, picks, scores[sl], lens[sl], fin[sl], EOS, table)
            newly += sum(1 for b in range(W) if f[b] and not fin[sl][p[b]])                             # beams that finish in this step
            fin[sl] = np.array(f, np.int32)
            anc[sl] = table_update(anc[sl], p, pos0 + t)
            parent += p
            cur += c
            live += W - int(fin[sl].sum())
        steps.append(dict(top_lp=top_lp, top_id=top_id, parent=parent, cur=cur, live=live, newly=newly, scores=scores.copy(), lens=lens.copy(), fin=fin.copy(),
                          anc=anc.copy()))
    return init, steps, margin


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("S,W,k", SHAPES)
def test_beam_select_eos_three_steps_against_numpy(K, S, W, k, alpha):  # noqa: F811
    """three consecutive steps on one state from *pos = 254 (the table columns cross one trip of the 256 threads), ids from a 40-id range
    that holds eos so beams finish on the way, sentences that start all finished, not at all and mixed, lengths that run past the
    table: tokens, parents, score bits, len, fin, the whole table, both logs, live, the ticket, the step counter and the position, exact"""
    init, steps, margin = eos_three_steps(S, W, k, alpha)
    print(f"S={S} W={W} k={k} alpha={alpha}: smallest Gumbel key margin of a live beam {margin:.3g}")
    assert margin >= 1e-3
    assert sum(s["newly"] for s in steps) > 0 or W == 1, "no beam finishes on the way"
    pos0, log_rows = 254, 2
    st = eos_state(K, S, W, log_rows, init["seeds"], EOS, init["table"])
    plog = torch.full((3, S * W), -5, dtype=torch.int32, device="cuda")                            # one row more than the state announces
    tlog = torch.full((3, S * W), -5, dtype=torch.int64, device="cuda")
    st.parent_log, st.tok_log = plog[:log_rows], tlog[:log_rows]
    st.anc.copy_(torch.from_numpy(init["anc"]))
    st.scores.copy_(torch.from_numpy(init["scores"]))
    st.len.copy_(torch.from_numpy(init["lens"]))
    st.fin.copy_(torch.from_numpy(init["fin"]))
    cur, pos = torch.empty(S * W, dtype=torch.int64, device="cuda"), i32(pos0)
    for t, want in enumerate(steps):
        K.beam_select_eos(dev(torch.from_numpy(want["top_lp"])), dev(torch.from_numpy(want["top_id"])), st, cur, pos, pos_inc=pos)
        assert int(st.ticket) == 0 and int(st.live_acc) == 0 and int(st.step) == t + 1 and int(pos) == pos0 + t + 1, t
        assert int(st.live) == want["live"], t
        assert cur.cpu().tolist() == want["cur"], t
        assert np.array_equal(st.scores.cpu().numpy().view(np.uint32), want["scores"].view(np.uint32)), t
        assert np.array_equal(st.len.cpu().numpy(), want["lens"]) and np.array_equal(st.fin.cpu().numpy(), want["fin"]), t
        assert np.array_equal(st.anc.cpu().numpy(), want["anc"]), t
        if t < log_rows:
            assert plog[t].cpu().tolist() == want["parent"] and tlog[t].cpu().tolist() == want["cur"], t
    assert bool((plog[log_rows:] == -5).all()) and bool((tlog[log_rows:] == -5).all())             # the third step wrote no log row


# =============================================================================================== 2. bit-equality with fk_beam_select_grouped
@pytest.mark.parametrize("eos", [EOS, -1], ids=["eos_absent", "eos=-1"])
@pytest.mark.parametrize("broadcast", [False, True], ids=["row_stride=k", "row_stride=0"])
@pytest.mark.parametrize("S,W,k", [(1, 4, 20), (3, 16, 20)])
def test_beam_select_eos_without_an_eos_equals_the_grouped_kernel(K, S, W, k, broadcast, eos):  # noqa: F811
    """no entry equal to eos, alpha = 0: three steps on twin states with the same seeds leave the same bits everywhere"""
    rng = np.random.default_rng(77 * S + W + (3 if broadcast else 0))
    seeds = [0x0BAD_5EED_0000_0000 + 31 * g for g in range(S)]
    a = K.BeamState("cuda", W, 3, TMAX, seed=seeds, groups=S)
    b = eos_state(K, S, W, 3, seeds, None if eos < 0 else eos, lenpow_table(8, 0.0))
    anc = torch.from_numpy(rng.integers(0, W, (S * W, TMAX)).astype(np.int32))
    sc = torch.from_numpy(np.concatenate([grid_rows(rng, 1, W)[0] for _ in range(S)]))
    for st in (a, b):
        st.anc.copy_(anc)
        st.scores.copy_(sc)
        st.parent_log.fill_(-5)
        st.tok_log.fill_(-5)
    cur_a, cur_b = (torch.empty(S * W, dtype=torch.int64, device="cuda") for _ in range(2))
    pos_a, pos_b = i32(254), i32(254)
    rows = S if broadcast else S * W
    for t in range(3):
        top_lp = dev(torch.from_numpy(grid_rows(rng, rows, k)))
        top_id = dev(torch.from_numpy(np.stack([2000 + rng.choice(40000, k, replace=False) for _ in range(rows)]).astype(np.int64)))
        K.beam_select_grouped(top_lp, top_id, a, cur_a, pos_a, pos_inc=pos_a, broadcast=broadcast)
        K.beam_select_eos(top_lp, top_id, b, cur_b, pos_b, pos_inc=pos_b, broadcast=broadcast)
        assert torch.equal(cur_a, cur_b) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)), t
        assert torch.equal(a.anc, b.anc) and torch.equal(a.parent_log, b.parent_log) and torch.equal(a.tok_log, b.tok_log), t
        assert int(a.step) == int(b.step) == t + 1 and int(pos_a) == int(pos_b) == 255 + t and int(b.ticket) == 0, t
        assert int(b.live) == S * W and int(b.fin.sum()) == 0 and bool((b.len == t + 1).all()), t


# =============================================================================================== 3. fixed point
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_all_finished_is_sorted_once_and_then_a_fixed_point(K, alpha):  # noqa: F811
    S, W, k = 2, 4, 10
    rng = np.random.default_rng(9)
    table = lenpow_table(12, alpha)
    st = eos_state(K, S, W, 2, [5, 6], EOS, table)
    st.anc.zero_()
    scores = np.concatenate([grid_rows(rng, 1, W)[0] for _ in range(S)])
    lens = rng.integers(1, 11, S * W).astype(np.int32)
    st.scores.copy_(torch.from_numpy(scores))
    st.len.copy_(torch.from_numpy(lens))
    st.fin.fill_(1)
    cur, pos = torch.empty(S * W, dtype=torch.int64, device="cuda"), i32(3)
    top_lp = dev(torch.from_numpy(grid_rows(rng, S * W, k)))
    top_id = dev(torch.from_numpy(np.stack([BASE + rng.choice(40, k, replace=False) for _ in range(S * W)]).astype(np.int64)))
    K.beam_select_eos(top_lp, top_id, st, cur, pos, pos_inc=pos)
    norm = scores * table[lens]
    want = np.concatenate([g * W + np.array(sorted(range(W), key=lambda b: (-norm[g * W + b], b))) for g in range(S)])
    assert np.array_equal(st.scores.cpu().numpy(), scores[want]) and np.array_equal(st.len.cpu().numpy(), lens[want])
    assert st.parent_log[0].cpu().tolist() == (want % W).tolist()
    first = (st.scores.clone(), st.len.clone(), st.fin.clone(), cur.clone())
    assert bool((cur == EOS).all()) and int(st.live) == 0 and bool((st.fin == 1).all())
    K.beam_select_eos(top_lp, top_id, st, cur, pos, pos_inc=pos)
    assert torch.equal(st.scores, first[0]) and torch.equal(st.len, first[1]) and torch.equal(st.fin, first[2]) and torch.equal(cur, first[3])
    assert st.parent_log[1].cpu().tolist() == list(range(W)) * S and bool((st.tok_log == EOS).all()) and int(st.live) == 0 and int(st.step) == 2


# =============================================================================================== 4. fk_beam_backtrack
def backtrack_ref(parent_log, tok_log, n, S, W, scores, lens, table, t0, cols, pad, prompt):
    ids = np.full((S, W, cols), pad, np.int64)
    ids[:, :, :t0] = prompt
    out_scores, out_len = np.zeros((S, W), np.float32), np.zeros((S, W), np.int32)
    for g in range(S):
        norm = [np.float32(scores[g * W + b] * table[min(max(int(lens[g * W + b]), 0), len(table) - 1)]) for b in range(W)]
        for rank, b in enumerate(sorted(range(W), key=lambda b: (-float(norm[b]), b))):
            out_scores[g, rank], out_len[g, rank] = scores[g * W + b], lens[g * W + b]
            x = b
            for t in range(n - 1, -1, -1):
                ids[g, rank, t0 + t] = tok_log[t, g * W + x]
                x = min(max(int(parent_log[t, g * W + x]), 0), W - 1)
    return ids, out_scores, out_len


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("step", [4, 6, 9])
def test_beam_backtrack_against_the_python_walk(K, step, alpha):  # noqa: F811
    """S = 3, W = 4, six log rows, a counter short of, at and past them; random parents, some outside [0, W) (clamped); a tie in the
    normalised scores (broken by beam number); one row longer than prompt + logs (padding even when all six steps count)"""
    S, W, log_rows, t0, cols, pad = 3, 4, 6, 2, 9, 777
    rng = np.random.default_rng(step)
    table = lenpow_table(8, alpha)
    st = eos_state(K, S, W, log_rows, [1, 2, 3], 5, table)
    parents = rng.integers(0, W, (log_rows, S * W)).astype(np.int32)
    parents[rng.integers(0, log_rows, 5), rng.integers(0, S * W, 5)] = np.array([-1, W, 99, -2 ** 31, 2 ** 31 - 1], np.int64).astype(np.int32)
    toks = rng.integers(0, 50257, (log_rows, S * W)).astype(np.int64)
    scores = np.concatenate([grid_rows(rng, 1, W)[0] for _ in range(S)])
    lens = rng.integers(1, 10, S * W).astype(np.int32)                                               # 8 and 9 lie past the table
    scores[1], lens[1] = scores[2], lens[2]                                                        # an exact tie inside sentence 0
    st.parent_log.copy_(torch.from_numpy(parents))
    st.tok_log.copy_(torch.from_numpy(toks))
    st.scores.copy_(torch.from_numpy(scores))
    st.len.copy_(torch.from_numpy(lens))
    st.step.fill_(step)
    prompt = np.array([11, 12], np.int64)
    ids = torch.full((S, W, cols), -3, dtype=torch.int64, device="cuda")
    ids[:, :, :t0] = torch.from_numpy(prompt).cuda()
    got_scores, got_len = K.beam_backtrack(st, ids, t0, pad)
    want_ids, want_scores, want_len = backtrack_ref(parents, toks, min(step, log_rows), S, W, scores, lens, table, t0, cols, pad, prompt)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(got_scores.cpu().numpy(), want_scores) and np.array_equal(got_len.cpu().numpy(), want_len)


# =============================================================================================== 5. fk_sample_topk_eos
def _sample_pair(K, logits, top_k, seed, step, eos, done, lens):  # noqa: F811
    B = logits.shape[0]
    a, b = K.SampleState("cuda", seed=seed, step=step), K.SampleState("cuda", seed=seed, step=step)
    es = K.SampleEosState("cuda", B, eos)
    es.done.copy_(torch.tensor(done, dtype=torch.int32))
    es.len.copy_(torch.tensor(lens, dtype=torch.int32))
    out_a, out_b = (torch.full((B, 6), -9, dtype=torch.int64, device="cuda") for _ in range(2))
    pos = i32(10)
    want = K.sample_topk(logits, 1.0, top_k, a, out=out_a)
    got = K.sample_topk_eos(logits, 1.0, top_k, b, es, out=out_b, pos_inc=pos)
    assert int(b.step) == step + 1 and int(b.ticket) == 0 and int(es.live_acc) == 0 and int(pos) == 11
    return want.cpu().tolist(), got.cpu().tolist(), out_a.cpu(), out_b.cpu(), es


def test_sample_topk_eos_done_rows_emit_eos_and_the_others_draw_as_before(K):  # noqa: F811
    B, V, top_k, eos = 5, 211, 10, 3
    buf = dev(rnd(B, V + 3, seed=12, scale=3.0))
    buf[:, eos] = -50.0                                                                            # far outside every row's top-10: never drawn
    logits = buf[:, :V]
    for step in (0, 2):
        want, got, out_a, out_b, es = _sample_pair(K, logits, top_k, 4242 + step, step, eos, [0, 1, 0, 1, 0], [2, 4, 0, 1, 3])
        live_rows = [0, 2, 4]
        assert [got[b] for b in (1, 3)] == [eos, eos] and [got[b] for b in live_rows] == [want[b] for b in live_rows]
        assert out_b[:, step].tolist() == got and bool((out_b[:, [c for c in range(6) if c != step]] == -9).all())
        assert all(want[b] != eos for b in live_rows)
        assert es.len.cpu().tolist() == [3, 4, 1, 1, 4] and es.done.cpu().tolist() == [0, 1, 0, 1, 0] and int(es.live) == 3
    # a row whose argmax is eos (top_k = 1) becomes done; so does a row that draws it at top_k = 10
    lg = logits.clone()
    lg[2, eos] = 50.0
    for k in (1, 10):
        want, got, _, _, es = _sample_pair(K, lg, k, 99, 1, eos, [0, 0, 0, 0, 1], [0, 0, 5, 0, 7])
        assert got[:4] == want[:4] and got[2] == eos and got[4] == eos
        assert es.done.cpu().tolist() == [0, 0, 1, 0, 1] and es.len.cpu().tolist() == [1, 1, 6, 1, 7] and int(es.live) == 3
    # eos = -1: nothing ever finishes
    want, got, _, _, es = _sample_pair(K, lg, 10, 99, 1, -1, [0] * 5, [0] * 5)
    assert got == want and int(es.live) == 5 and int(es.done.sum()) == 0


def test_sample_topk_eos_one_row_of_the_gpt2_vocabulary(K):  # noqa: F811
    logits = dev(rnd(1, 50257, seed=13, scale=3.0))
    want, got, _, _, es = _sample_pair(K, logits, 10, 7, 0, 50256, [0], [0])
    assert got == want and es.len.cpu().tolist() == [1] and int(es.live) == (0 if want[0] == 50256 else 1)
    top = int(logits.argmax())
    want, got, _, _, es = _sample_pair(K, logits, 1, 7, 0, top, [0], [0])
    assert got == want == [top] and es.done.cpu().tolist() == [1] and int(es.live) == 0


# =============================================================================================== 6. greedy collapse on the reference's tokens
def first_new_token(gen):
    """(j, token): the first generated token behind the first that does not occur earlier in the generated part"""
    j = next(j for j in range(1, len(gen)) if gen[j] not in gen[:j])
    assert j >= 2, j
    return j, int(gen[j])


def _check_greedy_eos(g, out, chain, t0, j, eos, W, same_bits=True):
    want = chain[:t0 + j + 1] + [eos] * (len(chain) - t0 - j - 1)
    assert out.cpu().tolist() == want
    assert g.last_beams == [want] * W and g.last_beam_lengths == [j + 1] * W
    assert len(set(g.last_beam_scores)) == 1 if same_bits else max(g.last_beam_scores) - min(g.last_beam_scores) <= 1e-4
    assert g.last_steps < 8 and g.last_steps <= (j + 1) + (j + 1) % 2, g.last_steps                 # j + 1 rounded up to the poll (every 2)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipGraph"])
@pytest.mark.parametrize("W", [3, 5])
def test_greedy_chain_stops_at_the_end_of_text_token(golden, fp32_mode, W, use_graph):  # noqa: F811
    g, zz, start, pf, _ = small_gpt(golden)
    chain = zz["tokens"].tolist()
    j, eos = first_new_token(chain[4:])
    out = g.generate_beam_search(start.clone(), 8, pf, topk=W, beam_width=W, use_cache=True, use_graph=use_graph, eos_token_id=eos, check_every=2)
    _check_greedy_eos(g, out, chain, 4, j, eos, W)


def test_re_forward_search_stops_at_the_end_of_text_token(golden, fp32_mode):  # noqa: F811
    """use_cache=False: the host loop with _beam_step_host and torch.multinomial draws (topk == W: every draw is the whole top-W)"""
    g, zz, start, pf, _ = small_gpt(golden)
    chain = zz["tokens"].tolist()
    j, eos = first_new_token(chain[4:])
    out = g.generate_beam_search(start.clone(), 8, pf, topk=3, beam_width=3, use_cache=False, eos_token_id=eos, check_every=2)
    _check_greedy_eos(g, out, chain, 4, j, eos, 3, same_bits=False)                                 # rows of one batched forward: equal within the logit tolerance


def test_greedy_chain_stops_at_the_end_of_text_token_gpt2_124m(model, z, fp32_mode):  # noqa: F811
    start, prefix = inputs_124m(z)
    chain = z["tokens"].tolist()
    j, eos = first_new_token(chain[1:])
    out = model.generate_beam_search(start.clone(), 8, prefix, topk=5, beam_width=5, use_cache=True, use_graph=True, eos_token_id=eos, check_every=2)
    _check_greedy_eos(model, out, chain, 1, j, eos, 5)


# =============================================================================================== 7. stochastic search against the host oracle
ALPHA7 = 1.0
# (torch seed, eos id) picked with the float64 CPU model of oracle/ (eos_host_oracle below on its logits): a beam finishes before the last
# step, another never does, and every decision stays >= 1.5x clear of its threshold there.  The test measures the margins again on the
# forward it runs and takes the first pair that qualifies.
CANDIDATES7 = [(2, 137), (4, 208), (8, 24), (8, 146), (14, 11)]


def eos_host_oracle(logits_fn, start_ids, seed, eos, alpha, W=W5, topk=TOPK5, new=NEW5, temperature=1.0):
    """tests/test_beam_gpu.py host_oracle with the end-of-text rules: logits_fn(beams [W, t] list) -> float64 last-position logits [W, V]
    of an un-cached forward; float64 log_softmax + topk, the Philox draws, eos_step_ref.  -> beams, raw scores, lengths, the step at which
    each final beam finished (None: never), and the smallest decision margin as a multiple of its threshold: 1e-3 at the top-k boundary
    and between the W-th and (W+1)-th Gumbel key of a live beam, ORDER_MARGIN inside the top-k of a live beam, and between neighbouring
    distinct candidates among the W + 1 best 1e-3 x inv_lenpow of the longer one (the two paths' logit error scales with that factor)"""
    table = lenpow_table(new + 2, alpha)
    beams, scores, lens, fin, margin = [list(start_ids)] * W, np.zeros(W, np.float32), [0] * W, [False] * W, np.inf
    ended = [None] * W
    for t in range(new):
        lp, ids = torch.log_softmax(logits_fn(beams) / temperature, -1).topk(topk + 1, -1)
        live = [i for i in range(W) if not fin[i]]
        if live:
            margin = min(margin, float((lp[live, topk - 1] - lp[live, topk]).min()) / 1e-3, float((lp[live, :-1] - lp[live, 1:]).min()) / ORDER_MARGIN)
        top_lp, top_id = lp[:, :topk].float().numpy(), ids[:, :topk].numpy()
        picks, key_margins = gumbel_draws(top_lp, t == 0, W, seed, t)
        margin = min([margin] + [key_margins[i] / 1e-3 for i in live])
        parent, tok, new_scores, new_lens, new_fin, cands = eos_step_ref(top_lp, top_id, t == 0, W, picks, scores, lens, fin, eos, table)
        ident = lambda c: tuple(beams[c[5]]) + (c[4],)                                              # a candidate is (history, token)
        for a, b in zip(cands[:W], cands[1:W + 1]):
            if ident(a) != ident(b):
                margin = min(margin, float(a[0] - b[0]) / (1e-3 * float(table[min(max(a[3], b[3]), len(table) - 1)])))
        ended = [ended[p] if fin[p] else (t if f else None) for p, f in zip(parent, new_fin)]
        beams, scores, lens, fin = [beams[p] + [c] for p, c in zip(parent, tok)], new_scores, new_lens, new_fin
    return beams, scores, lens, ended, margin


def _gpu_logits(g, pf, W):
    def fn(beams):
        with torch.no_grad():
            _, logits = g(torch.tensor(beams, device="cuda"), prefix=pf.expand(W, -1, -1).contiguous())
        return logits[:, -1, :].double().cpu()
    return fn


def _assert_best_first(scores, lens, alpha, new=NEW5):
    """last_beams / last_beam_scores / last_beam_lengths are ordered by score x inv_lenpow[length], the best first (fp32, the kernel's key)"""
    table = lenpow_table(new + 2, alpha)
    norm = [np.float32(np.float32(sc) * table[L]) for sc, L in zip(scores, lens)]
    assert all(a >= b for a, b in zip(norm, norm[1:])), norm


def test_cached_stochastic_search_with_eos_equals_the_host_oracle(golden, fp32_mode):  # noqa: F811
    """gpt_small, W = 4, topk = 10, 6 new tokens, alpha = 1: beams (as a set), lengths and raw scores (six log-probabilities, 1e-4 each)
    equal the host oracle's, eager and as a hipGraph, for the first committed (seed, eos) whose decisions are all clear of rounding"""
    g, zz, start, pf, _ = small_gpt(golden)
    assert 1 <= len(CANDIDATES7) <= 5
    for s, eos in CANDIDATES7:
        want_beams, want_scores, want_lens, ended, margin = eos_host_oracle(_gpu_logits(g, pf, W5), start[0].cpu().tolist(), seed_of(s), eos, ALPHA7)
        print(f"seed {s} eos {eos}: smallest decision margin {margin:.3g} x its threshold, beams finished at {ended}")
        if margin >= 1.0:
            break
    else:
        pytest.fail("none of the committed candidates keeps every decision clear of rounding")
    assert any(e is not None and e < NEW5 - 1 for e in ended), "no beam finishes before the last step"
    assert any(e is None for e in ended), "every beam finishes"
    want_order = sorted(range(W5), key=lambda b: want_beams[b])
    for use_graph in (False, True):
        torch.manual_seed(s)
        out = g.generate_beam_search(start.clone(), NEW5, pf, topk=TOPK5, beam_width=W5, use_cache=True, use_graph=use_graph, eos_token_id=eos,
                                     length_penalty=ALPHA7, check_every=2)
        assert sorted(g.last_beams) == sorted(want_beams), use_graph
        order = sorted(range(W5), key=lambda b: g.last_beams[b])
        assert [g.last_beam_lengths[b] for b in order] == [want_lens[b] for b in want_order]
        err = float(np.abs(np.array(g.last_beam_scores)[order] - want_scores[want_order]).max())
        print(f"graph={use_graph}: max |score - oracle| = {err:.3g}")
        assert err <= 6 * 1e-4
        assert out.cpu().tolist() == g.last_beams[0] and g.last_steps == NEW5
        _assert_best_first(g.last_beam_scores, g.last_beam_lengths, ALPHA7)


# =============================================================================================== 8. batched
# Three sentences, W = topk = 3 (every beam proposes its whole top-3, so nothing depends on the draws), 40 new tokens: the end-of-text id was
# picked with the float64 CPU model of oracle/ among the ids for which all beams of every sentence finish, at three different steps.
EOS8, NEW8 = 137, 40          # there: the sentences finish after 9, 31 and 7 steps, decisions >= 9.7e-4 apart


def test_batched_search_with_eos_equals_every_sentence_s_own_search(golden, fp32_mode):  # noqa: F811
    g, zz, _, _, _ = small_gpt(golden)
    starts, pf = three_sentences()
    seeds = [11, 12, 13]
    kw = dict(topk=3, beam_width=3, use_cache=True, eos_token_id=EOS8, length_penalty=0.6, check_every=1)
    alone = []
    for s in range(3):
        out = g.generate_beam_search(starts[s:s + 1].clone(), NEW8, pf[s:s + 1], seeds=seeds[s:s + 1], use_graph=False, **kw)
        alone.append((out.cpu().tolist(), g.last_beams, g.last_beam_lengths, g.last_beam_scores, g.last_steps))
    steps = [a[4] for a in alone]
    print(f"the sentences finish after {steps} steps")
    assert len(set(steps)) == 3 and max(steps) < NEW8, steps
    for use_graph in (False, True):
        out = g.generate_beam_search(starts.clone(), NEW8, pf, seeds=seeds, use_graph=use_graph, **kw)
        assert out.shape == (3, 4 + NEW8) and g.last_steps == max(steps)
        for s in range(3):
            assert out[s].cpu().tolist() == alone[s][0] and g.last_beams[s] == alone[s][1] and g.last_beam_lengths[s] == alone[s][2], (s, use_graph)
            np.testing.assert_allclose(g.last_beam_scores[s], alone[s][3], rtol=0, atol=NEW8 * 1e-4)


# The same with draws that matter (W = 4 of topk = 10, 6 new tokens, alpha = 1, one end-of-text id for the batch): per sentence up to five
# Philox seeds picked with the float64 CPU model of oracle/ so that every decision stays >= 1.5x clear of its threshold there (sentence 0: the
# seeds K.BeamState draws after torch.manual_seed(s); with these, beams of sentence 0 finish before the last step.  No id was found
# that the beams of all three sentences reach within six tokens, so the other two sentences only have to run beside a finishing one).
EOS8B = 137
SEEDS8B = [[2, 82, 235, 256, 294], [1000000, 1000002, 1000003, 1000005, 1000007], [2000001, 2000006, 2000007, 2000010, 2000012]]


def test_batched_stochastic_search_with_eos_equals_the_host_oracle_sentence_by_sentence(golden, fp32_mode):  # noqa: F811
    """every sentence of the batched search with `seeds` equals the host oracle of that sentence alone with its seed: beams as a set,
    lengths, raw scores within six log-probabilities of 1e-4, ordered best first, the returned row its best beam; eager and hipGraph"""
    g, zz, _, _, _ = small_gpt(golden)
    starts, pf = three_sentences()
    seeds, want, finished, never = [], [], [], 0
    for s in range(3):
        assert 1 <= len(SEEDS8B[s]) <= 5
        for cand in ([seed_of(x) for x in SEEDS8B[s]] if s == 0 else SEEDS8B[s]):
            beams, scores, lens, ended, margin = eos_host_oracle(_gpu_logits(g, pf[s:s + 1], W5), starts[s].cpu().tolist(), cand, EOS8B, ALPHA7)
            print(f"sentence {s} seed {cand}: smallest decision margin {margin:.3g} x its threshold, beams finished at {ended}")
            if margin >= 1.0:
                break
        else:
            pytest.fail(f"none of sentence {s}'s candidate seeds keeps every decision clear of rounding")
        seeds.append(cand)
        want.append((beams, scores, lens))
        finished += [e for e in ended if e is not None and e < NEW5 - 1]
        never += ended.count(None)
    assert finished and never, "the batch needs a beam that finishes before the last step and one that never does"
    for use_graph in (False, True):
        out = g.generate_beam_search(starts.clone(), NEW5, pf, topk=TOPK5, beam_width=W5, use_cache=True, use_graph=use_graph, seeds=seeds,
                                     eos_token_id=EOS8B, length_penalty=ALPHA7, check_every=2)
        assert out.shape == (3, 4 + NEW5)
        for s, (want_beams, want_scores, want_lens) in enumerate(want):
            got_beams, got_scores, got_lens = g.last_beams[s], g.last_beam_scores[s], g.last_beam_lengths[s]
            assert sorted(got_beams) == sorted(want_beams), (s, use_graph)
            order = sorted(range(W5), key=lambda b: got_beams[b])
            want_order = sorted(range(W5), key=lambda b: want_beams[b])
            assert [got_lens[b] for b in order] == [want_lens[b] for b in want_order], (s, use_graph)
            err = float(np.abs(np.array(got_scores)[order] - want_scores[want_order]).max())
            print(f"sentence {s} graph={use_graph}: max |score - oracle| = {err:.3g}")
            assert err <= 6 * 1e-4
            _assert_best_first(got_scores, got_lens, ALPHA7)
            assert out[s].cpu().tolist() == got_beams[0]


# =============================================================================================== 9. generate
def test_generate_stops_at_the_end_of_text_token_on_every_path(golden, fp32_mode):  # noqa: F811
    """top_k = 1 draws the argmax: the golden chain up to the end-of-text token of test 6, then padding, on the cached eager loop, the
    cached hipGraph and the re-forward loop"""
    g, zz, start, pf, _ = small_gpt(golden)
    chain, top_k = zz["tokens"].tolist(), 1
    assert chain == zz["tokens_argmax"].tolist()
    j, eos = first_new_token(chain[4:])
    want = chain[:4 + j + 1] + [eos] * (8 - j - 1)
    starts = start.repeat(2, 1)                                                                     # two rows: both stop at the same step
    for name, kw in (("eager", dict(use_graph=False)), ("graph", dict(use_graph=True)), ("re-forward", dict(use_cache=False))):
        out = g.generate(starts.clone(), 8, prefix=pf.expand(2, -1, -1).contiguous(), top_k=top_k, eos_token_id=eos, check_every=2, **kw)
        assert out.cpu().tolist() == want, name
        assert g.last_tokens.shape == (2, 12) and g.last_tokens.cpu().tolist() == [want] * 2, name
        assert g.last_lengths.cpu().tolist() == [j + 1] * 2 and g.last_steps < 8 and g.last_steps <= (j + 1) + (j + 1) % 2, (name, g.last_steps)


# =============================================================================================== 10. Franky
def test_franky_stop_trims_and_pads_and_the_defaults_are_unchanged(fp32_mode):  # noqa: F811
    """An untrained decoder never emits 50256, so its embedding row (tied to the head) gets a large random direction first: the logit of
    50256 is then huge at the steps where the hidden state points its way and far below the top-k elsewhere, and sentences end at
    different steps.  stop=False (or omitted) is the call as it was; stop=True trims a [T, C] call behind the first generated 50256 and
    pads a [S, T, C] call with it."""
    fr, x, gcfg = build_franky()
    fr.eval()
    eot, n_new = 50256, 7
    with torch.no_grad():
        w = fr.llm_model.lm_head.weight
        assert w.data_ptr() == fr.llm_model.transformer.wte.weight.data_ptr()
        w[eot] = 4.0 * torch.randn(w.shape[1], generator=torch.Generator().manual_seed(1)).to(w)
    # ---- sampling
    torch.manual_seed(4)
    probe = fr.generate(x[0].numpy(), max_new_tokens=n_new)
    torch.manual_seed(4)
    assert torch.equal(probe, fr.generate(x[0].numpy(), max_new_tokens=n_new, stop=False)) and probe.shape == (1 + n_new,)
    torch.manual_seed(4)
    one = fr.generate(x[0].numpy(), max_new_tokens=n_new, stop=True)
    gen = probe[1:].tolist()
    n = gen.index(eot) + 1 if eot in gen else n_new
    assert one.tolist() == probe[:1 + n].tolist() and int(fr.last_lengths[0]) == n                 # the same draws, cut behind the first 50256
    many = fr.generate(x[:3].numpy(), max_new_tokens=n_new, stop=True)
    lengths = fr.last_lengths.tolist()
    assert many.shape == (3, 1 + n_new) and len(lengths) == 3 and bool((many[:, 0] == eot).all())
    for s in range(3):
        assert bool((many[s, 1 + lengths[s]:] == eot).all()) and eot not in many[s, 1:lengths[s]].tolist()
        assert lengths[s] == n_new or int(many[s, lengths[s]]) == eot
    assert min(lengths) < n_new, "no sentence ended early: the test needs another direction"
    # ---- beam search
    torch.manual_seed(3)
    probe = fr.generate_beam(x[0].numpy(), max_new_tokens=n_new)
    torch.manual_seed(3)
    assert torch.equal(probe, fr.generate_beam(x[0].numpy(), max_new_tokens=n_new, stop=False, length_penalty=0.0)) and probe.shape == (1 + n_new,)
    one = fr.generate_beam(x[0].numpy(), max_new_tokens=n_new, stop=True, length_penalty=0.6)
    n = int(fr.last_lengths[0])
    assert one.dim() == 1 and one.shape[0] == 1 + n and int(one[0]) == eot and eot not in one[1:n].tolist()
    assert n == n_new or int(one[n]) == eot
    for kw in ({}, {"batch_sentences": 2}):
        many = fr.generate_beam(x[:3].numpy(), max_new_tokens=n_new, stop=True, **kw)
        lengths = fr.last_lengths.tolist()
        assert many.shape == (3, 1 + n_new) and len(lengths) == 3 and bool((many[:, 0] == eot).all())
        for s in range(3):
            assert bool((many[s, 1 + lengths[s]:] == eot).all()) and eot not in many[s, 1:lengths[s]].tolist()
            assert lengths[s] == n_new or int(many[s, lengths[s]]) == eot
        assert min(lengths) < n_new


# =============================================================================================== 11. the one step loop; the two re-forward loops against each other
@pytest.mark.parametrize("check_every", [1, 3, 8])
def test_run_steps_counts_alike_eager_and_as_a_graph(check_every):
    """GPT._run_steps with a step of torch ops (no project kernel): every (max_new_tokens, die) of tests/test_decode_loop_cpu.py, eager on
    the current stream and as warm-up + capture + replays; both stop where the arithmetic says and run exactly the steps they report."""
    for max_new_tokens, ce, die in LOOP_CASES:
        if ce != check_every:
            continue
        want = expected_steps(max_new_tokens, check_every, die)
        eager = run_counted("cuda", max_new_tokens, check_every, die, use_graph=False)
        graph = run_counted("cuda", max_new_tokens, check_every, die, use_graph=True)
        assert eager == graph == (want, want - 1), (max_new_tokens, check_every, die, eager, graph)
    for max_new_tokens in (1, 2, 3, 4, 9):
        for use_graph in (False, True):
            assert run_counted("cuda", max_new_tokens, None, 1, use_graph=use_graph, poll=False) == (max_new_tokens, max_new_tokens - 1)


def test_plain_re_forward_search_is_the_end_of_text_loop_with_an_id_that_is_never_drawn(golden, fp32_mode):  # noqa: F811
    """use_cache=False, gpt_small, W = 3, topk = 6, 6 new tokens, one torch seed: the call without an end-of-text id returns what the call
    with one returns whose id no beam holds (same forwards, same torch.multinomial draws, the same selection with nothing finished), and it
    records nothing.  The two calls run two loops (the tail of generate_beam_search and _beam_search_host_eos): this pins them to each other."""
    g, zz, start, pf, _ = small_gpt(golden)
    g.last_beams = None
    torch.manual_seed(20260)
    plain = g.generate_beam_search(start.clone(), 6, pf, topk=6, beam_width=3, use_cache=False)
    assert g.last_beams is None
    for eos in (210, 0, 1, 2, 105, 209):
        torch.manual_seed(20260)
        out = g.generate_beam_search(start.clone(), 6, pf, topk=6, beam_width=3, use_cache=False, eos_token_id=eos, length_penalty=0.0)
        if all(tok != eos for beam in g.last_beams for tok in beam):
            break
    else:
        pytest.fail("every candidate id occurs in some beam")
    assert plain.shape == (4 + 6,) and torch.equal(plain, out)
    assert g.last_steps == 6 and len(g.last_beams) == 3
