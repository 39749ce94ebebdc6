"""Every draw of the one-launch sampler on the MI355X against the float64 restatement of its rule (tests/sample_ref.py): fk_sample_topk,
fk_sample_topk_eos and fk_sample_topp (plain and end-of-text mode), at every case of tests/sample_cases.py, and GPT.generate on the small
golden GPT, teacher-forced on its own output.

The draw is a pure function of (logits, temperature, top_k, top_p, seed, step, row), so nothing here is a statistic: EVERY draw must lie in
its accepted set, the tokens within EPS = 2^-17 of the total mass of u * total (tests/sample_ref.py derives it), and equal the reference's
token wherever that set has one member (>= 95 % of the draws of every case, tests/test_sample_draws_cpu.py).  The device buffer of a case
has row stride V rounded up to 8, plus 8, and NaN behind V: a NaN key sorts above +inf and a NaN term poisons the sum, so one read past V
changes the draws.  Per launch: the step counter advanced by exactly one (across 2^32 + 5 too), pos_inc by one, the ticket back at 0,
out[:, step] == cur while step < out_cols and nothing else of `out` touched, logits and NaN columns bit for bit as they were.

Every launch prints `EXC <case> <entry point> <largest excursion>`: the distance of u * total from the drawn token's interval in units of
EPS * total over the launch's draws, 0 inside.  An excursion above 1 fails.  Largest per entry point on the MI355X:
    sample_topk 0.013, sample_topk_eos 0.013, sample_topp (plain and end-of-text mode) 0.013, all on v50257-placed-p45 drawn at top_p = 1
    (v50257-placed 0.010, v50257-kV 0.004, every other case 0.000: no draw left its own interval);
    generate, generate + top_p, generate + top_p + end-of-text id: 0.000 (24, 24 and 25 draws; torch seeds 1, 2, 3)."""
import numpy as np
import pytest
import torch

import frankenstein_amd as fa  # noqa: F401
from tests import sample_cases as SC
from tests import sample_ref as R
from tests.test_beam_gpu import K, fp32_mode, i32, seed_of, small_gpt  # noqa: F401

pytestmark = pytest.mark.gpu

OUT_COLS = 4
EOS_LEN0 = 5            # the length a row that starts done carries in


class Loaded:
    def __init__(self, case):
        self.case = case
        self.rows = SC.logits_of(case)
        stride = (case.V + 7) // 8 * 8 + 8
        self.host = np.full((case.B, stride), np.nan, np.float32)
        self.host[:, :case.V] = self.rows
        self.wide = torch.from_numpy(self.host).cuda()
        self.logits = self.wide[:, :case.V]
        self._refs = {}

    def refs(self, top_p):
        if top_p not in self._refs:
            self._refs[top_p] = SC.refs_of(self.case, self.rows, top_p)
        return self._refs[top_p]

    def assert_inputs_untouched(self):
        assert np.array_equal(self.wide.cpu().numpy().view(np.uint32), self.host.view(np.uint32)), "the launch wrote to its logits or behind them"


@pytest.fixture(scope="module", params=SC.CASES, ids=lambda c: c.name)
def loaded(request):
    """module scope: the tests of one case run next to each other and share its buffer and its references"""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return Loaded(request.param)


def run(K, L, entry, top_p=1.0, eos_mode=None, launches=1):  # noqa: F811
    """`launches` consecutive launches of one entry point on one fresh state, every draw and every side effect checked.
    eos_mode: None (no end-of-text state), "live" (no row done), "thirds" (every third row starts done)"""
    case, B = L.case, L.case.B
    refs = L.refs(top_p)
    eos = min(3, case.V - 1)
    state = K.SampleState("cuda", seed=case.seed, step=case.step)
    pos = i32(11)
    out = torch.full((B, OUT_COLS), -7, dtype=torch.int64, device="cuda")
    cur = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    es, done0 = None, np.zeros(B, bool)
    if eos_mode is not None:
        es = K.SampleEosState("cuda", B, eos)
        if eos_mode == "thirds":
            done0[::3] = True
            es.done.copy_(torch.from_numpy(done0.astype(np.int32)))
            es.len.copy_(torch.from_numpy(np.where(done0, EOS_LEN0, 0).astype(np.int32)))
    assert launches == 1 or es is None
    want_out = out.cpu().numpy()
    worst = 0.0
    for n in range(launches):
        if entry == "sample_topk":
            ret = K.sample_topk(L.logits, case.T, case.top_k, state, cur=cur, out=out, pos_inc=pos)
        elif entry == "sample_topk_eos":
            ret = K.sample_topk_eos(L.logits, case.T, case.top_k, state, es, cur=cur, out=out, pos_inc=pos)
        else:
            ret = K.sample_topp(L.logits, case.T, case.top_k, top_p, state, es, cur=cur, out=out, pos_inc=pos)
        assert ret is cur
        got = cur.cpu().numpy()
        step = case.step + n
        assert int(state.step) == step + 1 and int(pos) == 12 + n and int(state.ticket) == 0
        if step < OUT_COLS:
            want_out[:, step] = got
        assert np.array_equal(out.cpu().numpy(), want_out), "out[:, step] is cur while step < out_cols, and nothing else moves"
        us = SC.uniforms_of(case, n)
        live = np.nonzero(~done0)[0]
        label = f"{case.name} {entry} p={top_p} {eos_mode or 'plain'} launch {n}"
        exc = R.assert_draws([refs[b] for b in live], [us[b] for b in live], got[live], label) if live.size else 0.0
        worst = max(worst, exc)
        if es is not None:
            assert (got[done0] == eos).all(), "a done row emits the id"
            lens, done = es.len.cpu().numpy(), es.done.cpu().numpy()
            assert (lens[done0] == EOS_LEN0).all() and (lens[~done0] == 1).all(), "a done row keeps its length, a live one grows by one"
            assert np.array_equal(done != 0, done0 | (got == eos)), "a row that draws the id becomes done"
            assert int(es.live) == int((~done0 & (got != eos)).sum()) and int(es.live_acc) == 0
    L.assert_inputs_untouched()
    print(f"EXC {case.name} {entry}{'' if entry != 'sample_topp' else f'@{top_p}'}{'' if eos_mode is None else '/' + eos_mode} {worst:.3f}")
    return worst


# =============================================================================================== kernel level
def test_sample_topk_draws_the_references_tokens(K, loaded):  # noqa: F811
    """two consecutive steps on one state (top_p cases: sample_topk has no nucleus, the reference at top_p = 1)"""
    run(K, loaded, "sample_topk", launches=SC.LAUNCHES)


def test_sample_topk_eos_draws_the_references_tokens(K, loaded):  # noqa: F811
    """no row done: every row draws sample_topk's token; every third row done: those emit the id and keep their length, the others draw
    the reference's token for their own row index"""
    run(K, loaded, "sample_topk_eos", eos_mode="live")
    run(K, loaded, "sample_topk_eos", eos_mode="thirds")


def test_sample_topp_draws_the_references_tokens(K, loaded):  # noqa: F811
    """top_p = 1 must draw what sample_topk draws (the same reference), top_p < 1 from the nucleus; plain and end-of-text mode"""
    for top_p in sorted({1.0, loaded.case.top_p}, reverse=True):
        run(K, loaded, "sample_topp", top_p=top_p)
        run(K, loaded, "sample_topp", top_p=top_p, eos_mode="thirds")


def test_the_check_notices_draws_of_another_step(K):  # noqa: F811
    """the tokens of step 0 judged as if they were step 1's: nearly all of them fall outside (the harness compares what it says it does)"""
    L = Loaded(SC.BY_NAME["v1000-normal"])
    state = K.SampleState("cuda", seed=L.case.seed, step=0)
    got = K.sample_topk(L.logits, L.case.T, L.case.top_k, state).cpu().numpy()
    assert not R.judge(L.refs(1.0), SC.uniforms_of(L.case, 0), got)[0]
    assert len(R.judge(L.refs(1.0), SC.uniforms_of(L.case, 1), got)[0]) > 0.9 * L.case.B


# =============================================================================================== model level
NEW = 24
TOP_K, TEMPERATURE, TOP_P = 20, 0.8, 0.9
# The logits of a model cannot be shaped, so its nucleus boundary lies where it lies: include/franken_hip.h lets a token whose
# |mass_gt / total - top_p| is below 1e-4 fall on either side, and a step is judged only with twice that clear.  gpt_small's top 20 hold
# about .05 each, so a boundary comes within 2e-4 of .9 at under 1 % of the steps; a torch seed with such a step is passed over, and
# the first of these that has none is the one judged.
MODEL_MARGIN = 2e-4
MODEL_SEEDS = [1, 2, 3, 4, 5, 6, 7, 8]


def teacher_forced(g, pf, tokens, t0, steps, seed, top_p, lengths=None):
    """tokens [B, t0 + NEW] as the model emitted them.  For every step t < steps and every row b still drawing (t < lengths[b]): the last
    fp32 logits row of the forward of tokens[:, :t0 + t], the same batch the re-forward loop ran, and the token emitted there against the
    reference for (seed, step = t, row = b).  -> the largest excursion; raises R.MarginError where a nucleus boundary is too close"""
    B = tokens.shape[0]
    rows, us, got = [], [], []
    for t in range(steps):
        with torch.no_grad():
            _, lg = g(tokens[:, :t0 + t].contiguous(), prefix=pf)
        last = lg[:, -1, :].float().cpu().numpy()
        for b in range(B):
            if lengths is None or t < lengths[b]:
                rows.append(R.row_ref(np.ascontiguousarray(last[b]), TEMPERATURE, TOP_K, top_p, MODEL_MARGIN))
                us.append(R.uniform(seed, t, b))
                got.append(int(tokens[b, t0 + t]))
    return R.assert_draws(rows, us, got, f"generate top_p={top_p}"), len(got)


def first_seed_that_is_clear(check):
    for s in MODEL_SEEDS:
        try:
            return s, check(s)
        except R.MarginError as e:
            print(f"torch seed {s} passed over: {e}")
    raise AssertionError(f"none of the torch seeds {MODEL_SEEDS} keeps every nucleus boundary {MODEL_MARGIN} clear of top_p: extend the list")


@pytest.mark.parametrize("top_p", [None, TOP_P], ids=["top_k", "top_k+top_p"])
def test_generate_emits_the_references_token_at_every_step(golden, fp32_mode, top_p):  # noqa: F811
    g, _, start, pf, _ = small_gpt(golden)
    t0 = start.shape[1]

    def check(s):
        seed = seed_of(s)                                   # the torch.randint SampleState makes behind torch.manual_seed(s)
        torch.manual_seed(s)
        out = g.generate(start.clone(), NEW, prefix=pf, temperature=TEMPERATURE, top_k=TOP_K, top_p=top_p, use_cache=False)
        assert out.shape == (t0 + NEW,)
        return teacher_forced(g, pf, out[None, :], t0, NEW, seed, 1.0 if top_p is None else top_p)

    s, (worst, n) = first_seed_that_is_clear(check)
    print(f"EXC generate{'' if top_p is None else '+top_p'} seed={s} draws={n} {worst:.3f}")
    assert n == NEW


def test_generate_with_an_end_of_text_id_emits_the_references_tokens_until_each_row_ends(golden, fp32_mode):  # noqa: F811
    """three rows of the same prompt (the row index keys the draw, so they part at once); the id is the first token row 0 draws from its
    seventh step on that it has not drawn before, so row 0 ends inside the call.  Behind its id a row emits the id and draws nothing"""
    g, _, start, pf, _ = small_gpt(golden)
    B, t0 = 3, start.shape[1]
    starts, pf3 = start.repeat(B, 1), pf.expand(B, -1, -1).contiguous()
    kw = dict(prefix=pf3, temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, use_cache=False)

    def check(s):
        seed = seed_of(s)
        torch.manual_seed(s)
        probe = g.generate(starts.clone(), NEW, **kw)[t0:].tolist()          # row 0 without an id: the same draws up to it
        j = next((j for j in range(6, NEW - 1) if probe[j] not in probe[:j]), NEW - 1)
        eos = probe[j]
        torch.manual_seed(s)
        out = g.generate(starts.clone(), NEW, eos_token_id=eos, check_every=4, **kw)
        tokens, lengths = g.last_tokens, g.last_lengths.cpu().tolist()
        assert tokens.shape == (B, t0 + NEW) and torch.equal(out, tokens[0]) and lengths[0] == j + 1
        assert tokens[0, t0:].tolist() == probe[:j + 1] + [eos] * (NEW - j - 1)
        for b in range(B):
            gen = tokens[b, t0:].tolist()
            assert gen[lengths[b]:] == [eos] * (NEW - lengths[b]) and eos not in gen[:lengths[b] - 1], b
            assert lengths[b] == NEW or gen[lengths[b] - 1] == eos, b
        return teacher_forced(g, pf3, tokens, t0, max(lengths), seed, TOP_P, lengths)

    s, (worst, n) = first_seed_that_is_clear(check)
    print(f"EXC generate+top_p+eos seed={s} draws={n} {worst:.3f}")
