"""Repetition penalty, n-gram ban and minimum length on the MI355X: fk_logit_rules against the loop-by-loop restatement of its rule
(tests/test_logit_rules_cpu.py rules_ref), bit for bit, with the token history it keeps on the device; the sampler never emits a token
without mass; and GPT.generate / generate_beam_search / Franky give the same ruled tokens on every path.

The model tests decode greedily (top_k = 1, or topk == beam_width, where the search collapses to its greedy chain) in fp32 on gpt_small:
with the float64 CPU model of oracle/ the two best ruled candidates of every step below lie at least 2.8e-3 apart, 14 x ORDER_MARGIN."""
import numpy as np
import pytest
import torch

from tests import cases as C
from tests.test_beam_gpu import ORDER_MARGIN, K, build_franky, fp32_mode, small_gpt  # noqa: F401  (fixtures)
from tests.test_logit_rules_cpu import rules_ref

pytestmark = pytest.mark.gpu

SENT = 12345.0          # behind column V of every logits row
HSENT = -7              # in every history column nobody has written yet

# every rule alone, and all three together: (p, n, m, e)
RULESETS = {"penalty": (1.3, 0, 0, -1), "ngram": (1.0, 3, 0, -1), "minlen": (1.0, 0, 300, 4), "all": (0.8, 2, 300, 4)}


def mk_rules(K, prompt, steps, p, n, m, e, width=None):  # noqa: F811
    return K.LogitRules(prompt.cuda(), steps, p, n, m, None if e < 0 else e, width)


def want_rows(z, hist, g, p, n, m, e):
    return torch.from_numpy(np.stack([rules_ref(z[r], hist[r], g, p, n, m, e) for r in range(len(hist))]))


def token_stream(R, V, n, seed):
    """[R, n] ids: mostly from six tokens (duplicates, repeated n-grams), the rest anywhere, token 0 and token V - 1 included"""
    g = torch.Generator().manual_seed(seed)
    few = torch.tensor([0, V - 1, 4, 5, 17 % V, V // 2])[torch.randint(0, 6, (R, n), generator=g)]
    return torch.where(torch.rand(R, n, generator=g) < 0.75, few, torch.randint(0, V, (R, n), generator=g))


# =============================================================================================== 1. the kernel, plain mode
@pytest.mark.parametrize("V", [70, 512, 50257])
@pytest.mark.parametrize("R", [1, 5, 17])
def test_logit_rules_plain_mode_against_the_restatement(K, R, V):  # noqa: F811
    """Histories of L = 0, 1, 2 (an empty prompt, then two appends) and of L = 2 .. 600 (a prompt of two out-of-range ids, then 598 appends
    through consecutive launches on one state, two of them ids the sampler could never have written): the history buffer is checked after
    every launch, the logits bit for bit at L in {0, 1, 2, 255, 256, 257, 600}, the columns behind V (ld = V + 3) are never touched"""
    CHECK = {0, 1, 2, 255, 256, 257, 600}
    for name, (p, n, m, e) in RULESETS.items():
        for t0, steps, prompt in ((0, 2, torch.empty((R, 0), dtype=torch.int64)), (2, 598, torch.tensor([[-1, V]]).repeat(R, 1))):
            toks = token_stream(R, V, steps, seed=R * 1000 + V + t0)
            if steps > 300:
                toks[:, 100], toks[:, 200] = V, -5                                                 # not tokens: the kernel files them as -1
            hist = torch.cat([prompt, torch.where((toks >= 0) & (toks < V), toks, torch.full_like(toks, -1))], 1)      # the walk, all at once
            hist_dev, toks_dev = hist.to(torch.int32).cuda(), toks.cuda()
            lr = mk_rules(K, prompt, steps, p, n, m, e)
            lr.hist[:, t0:] = HSENT
            zg = torch.Generator().manual_seed(V + R)
            z = torch.randn(R, V, generator=zg) * 3
            z[:, [0, V - 1]] = torch.tensor([1.5, -2.5])
            fresh = torch.full((R, V + 3), SENT)
            fresh[:, :V] = z
            fresh = fresh.cuda()
            buf = fresh.clone()
            step = torch.zeros(1, dtype=torch.int64, device="cuda")
            cur = torch.full((R,), 3, dtype=torch.int64, device="cuda")
            for s in range(steps + 1):
                L = t0 + s
                if s > 0:
                    cur.copy_(toks_dev[:, s - 1])
                    step.fill_(s)
                if L in CHECK:
                    buf.copy_(fresh)
                K.logit_rules_(buf[:, :V], lr, step, cur)
                assert torch.equal(lr.hist[:, :L], hist_dev[:, :L]) and bool((lr.hist[:, L:] == HSENT).all()), (name, L)
                if L in CHECK:
                    got = buf.cpu()
                    assert torch.equal(got[:, :V], want_rows(z.numpy(), hist[:, :L].tolist(), s, p, n, m, e)), (name, L)
                    assert bool((got[:, V:] == SENT).all()), (name, L)


def test_logit_rules_plain_mode_ignores_a_step_counter_outside_its_history(K):  # noqa: F811
    """*step < 0 or t0 + *step past the row: nothing is written, neither the rows in front of and behind the history nor the logits"""
    R, V, t0, steps = 3, 70, 2, 4
    lr = mk_rules(K, torch.tensor([[5, 6]]).repeat(R, 1), steps, 1.3, 1, 9, 4)
    big = torch.full((R + 2, t0 + steps), HSENT, dtype=torch.int32, device="cuda")
    big[1:-1, :t0] = lr.hist[:, :t0]
    lr.hist = big[1:-1]
    before = big.clone()
    z = torch.randn(R, V, generator=torch.Generator().manual_seed(1)).cuda()
    cur = torch.full((R,), 9, dtype=torch.int64, device="cuda")
    for s in (-1, steps + 1, steps + 50, 1 << 40):
        buf = z.clone()
        K.logit_rules_(buf, lr, torch.tensor([s], dtype=torch.int64, device="cuda"), cur)
        assert torch.equal(big, before) and torch.equal(buf, z), s
    buf = z.clone()
    K.logit_rules_(buf, lr, torch.tensor([steps], dtype=torch.int64, device="cuda"), cur)          # the last column is the kernel's
    assert torch.equal(big[1:-1, -1].cpu(), torch.full((R,), 9, dtype=torch.int32)) and bool((big[[0, -1]] == HSENT).all())
    assert not torch.equal(buf, z)


# =============================================================================================== 2. the kernel, beam mode
def test_logit_rules_beam_mode_follows_the_parents(K):  # noqa: F811
    """S = 2 sentences x W = 3 beams, a prompt of 2 tokens, five steps (the first with one logits row per sentence), hand-written parents: a
    parent kept twice, a beam dropped, corrupt parents (clamped into the sentence).  Every row's history after every step is the Python
    walk, the logits are the restatement of that history; a step counter past the logs or past the history writes nothing."""
    S, W, V, t0, steps = 2, 3, 70, 2, 5
    p, n, m, e = 1.3, 2, 3, 5
    prompt = torch.tensor([[7, 8], [9, 7]])
    parents = [[0, 0, 0, 2, 1, 0],            # written by step 0 (all beams are the sentence's one sequence)
               [0, 0, 2, 1, 1, 1],            # sentence 0: beam 0 kept twice, beam 1 dropped; sentence 1: only beam 1 survives
               [2, 7, -3, 0, 100, -1],        # corrupt: 7 -> 2, -3 -> 0, 100 -> 2, -1 -> 0
               [1, 1, 0, 2, 2, 0]]
    toks = [[8, 7, 8, 7, 9, 7], [7, 8, 8, 9, 7, 7], [8, 8, 7, 5, 9, 9], [7, 5, 8, 7, 7, 9], [0, 69, 8, 9, 9, 7]]      # cur after step s
    lr = mk_rules(K, prompt, steps, p, n, m, e, width=W)
    big = torch.full((2, S * W + 2, t0 + steps), HSENT, dtype=torch.int32, device="cuda")         # a guard row in front of and behind each buffer
    big[0, 1:-1, :t0] = lr.hist[:, :t0]
    lr.hist, lr.hist2 = big[0, 1:-1], big[1, 1:-1]
    parent_log = torch.tensor(parents, dtype=torch.int32).cuda()                                   # 4 rows: steps 1 .. 4 read rows 0 .. 3
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    cur = torch.full((S * W,), 11, dtype=torch.int64, device="cuda")
    z = torch.randn(S * W, V, generator=torch.Generator().manual_seed(2)) * 3
    walk = [prompt[r // W].tolist() for r in range(S * W)]
    for s in range(steps):
        rows = S if s == 0 else S * W
        if s > 0:
            walk = [walk[(r // W) * W + min(max(parents[s - 1][r], 0), W - 1)] + [toks[s - 1][r]] for r in range(S * W)]
            cur.copy_(torch.tensor(toks[s - 1]))
            step.fill_(s)
        buf = torch.full((rows, V + 3), SENT)
        buf[:, :V] = z[:rows]
        buf = buf.cuda()
        K.logit_rules_(buf[:, :V], lr, step, cur, parent_log, broadcast=s == 0)
        new = (lr.hist2 if s & 1 else lr.hist)[:, :t0 + s].cpu().tolist()
        assert new == walk, (s, new, walk)
        hist = [walk[g * W] for g in range(S)] if s == 0 else walk
        got = buf.cpu()
        assert torch.equal(got[:, :V], want_rows(z.numpy(), hist, s, p, n, m, e)) and bool((got[:, V:] == SENT).all()), s
        assert bool((big[:, [0, -1]] == HSENT).all()) and bool((big[:, :, t0 + s:] == HSENT).all()), s
    before = big.clone()
    for s in (steps, steps + 1, -2):            # past the logs (4 rows: *step = 5 would read row 4), past the history, negative
        step.fill_(s)
        buf = z.clone().cuda()
        K.logit_rules_(buf, lr, step, cur, parent_log)
        assert torch.equal(big, before) and torch.equal(buf.cpu(), z), s


# =============================================================================================== 3. the sampler never emits a token without mass
@pytest.mark.parametrize("top_k", [None, 50])
def test_sampler_never_draws_a_token_without_mass(K, top_k):  # noqa: F811
    """2048 rows x 10 launches of one row with 7 finite logits among 5000 (5 per thread of the sampler, the last ones of every chunk and of
    the row -inf; top_k = 50 > 7 keeps -inf entries as well): every draw is one of the 7, whichever entry point draws it.  And the -inf
    entries do not move a draw: the tokens are those K.sample_topk draws from the 7 finite logits alone, same seed, same steps."""
    V, B, n = 5000, 2048, 10
    pos = torch.tensor([1, 6, 7, 2503, 2504, 4990, 4996])
    vals = torch.tensor([0.5, 1.5, -0.5, 2.0, 1.0, 0.0, 1.75])
    row = torch.full((V,), -float("inf"))
    row[pos] = vals
    lg = row.expand(B, V).contiguous().cuda()
    small = vals.expand(B, 7).contiguous().cuda()
    draws = {}
    for name in ("topk", "topk_eos", "topp", "compact"):
        st = K.SampleState("cuda", seed=77)
        out = torch.empty((B, n), dtype=torch.int64, device="cuda")
        es = K.SampleEosState("cuda", B, None)
        for _ in range(n):
            if name == "topk":
                K.sample_topk(lg, 0.9, top_k, st, out=out)
            elif name == "topk_eos":
                K.sample_topk_eos(lg, 0.9, top_k, st, es, out=out)
            elif name == "topp":
                K.sample_topp(lg, 0.9, top_k, 0.999, st, out=out)
            else:
                K.sample_topk(small, 0.9, None, st, out=out)
        draws[name] = out.cpu()
    for name in ("topk", "topk_eos", "topp"):
        assert bool(torch.isin(draws[name], pos).all()), name
    assert torch.equal(draws["topk"], pos[draws["compact"]]) and torch.equal(draws["topk_eos"], draws["topk"])
    assert sorted(set(draws["topk"].view(-1).tolist())) == sorted(pos.tolist())                   # and all seven are drawn


def test_sampler_fallback_scan_skips_entries_without_mass(K):  # noqa: F811
    """The draws above reach the sampler's fallback (the owning thread's running mass ends at or below the target) about once in 1e7, so
    they would pass without the change to it.  This row forces it: token 0 holds the maximum (mass 1), every other kept token a mass of
    2^-25, below half an ulp of 1, and V = 1024 x 512 gives every thread of the sampler a chunk of 512 whose last entry is -inf.  The
    sequential sum inside a chunk then never moves (1 + 2^-25 = 1 in fp32) while the scan of the chunk sums (511 x 2^-25 each) does, so
    every target >= 1, 1.5 % of the draws, ends in the fallback of its owning thread.  That scan used to answer "the last kept index",
    the -inf entry at the end of the chunk; it must answer the last index WITH mass, the one in front of it.  (The second fallback, the
    backward scan of thread 0, needs target >= total, which u < 1 never gives in fp32; it is changed the same way and not reached here.)"""
    chunk, B, n = 512, 128, 64
    V = 1024 * chunk
    row = torch.full((V,), -25.0 * float(np.log(2.0)), device="cuda")
    row[chunk - 1::chunk] = -float("inf")
    row[0] = 0.0
    lg = row.repeat(B, 1)
    for name in ("topk", "topk_eos"):
        st = K.SampleState("cuda", seed=4242)
        es = K.SampleEosState("cuda", B, None)
        out = torch.empty((B, n), dtype=torch.int64, device="cuda")
        for _ in range(n):
            if name == "topk":
                K.sample_topk(lg, 1.0, None, st, out=out)
            else:
                K.sample_topk_eos(lg, 1.0, None, st, es, out=out)
        tok = out.view(-1)
        assert bool(torch.isfinite(row[tok]).all()), (name, tok[~torch.isfinite(row[tok])][:8].tolist())
        late = tok[tok != 0]
        print(f"{name}: {late.numel()} of {tok.numel()} draws took the fallback")
        assert late.numel() >= 20                                          # expected 8192 x 1.5 % = 126: the fallback is what this test is about
        assert bool((late % chunk == chunk - 2).all())                     # the last token with mass of the owning thread's chunk


# =============================================================================================== 4. the model: every path agrees
NEW = 12
MODEL_RULES = {"penalty": dict(repetition_penalty=1.3), "ngram": dict(no_repeat_ngram_size=2), "minlen": dict(min_new_tokens=4, eos_token_id=24),
               "all": dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4, eos_token_id=24)}


def ref_kw(kw):
    return dict(p=kw.get("repetition_penalty", 1.0), n=kw.get("no_repeat_ngram_size", 0), m=kw.get("min_new_tokens", 0), e=kw.get("eos_token_id", -1))


def loop_chain(g, start, pf, n_new, **kw):
    """the decode loop written out: un-cached forward, rules_ref on its last-position logits, argmax; a row that emits the id is done.
    -> the tokens and the smallest gap between the two best ruled candidates"""
    cur, margin, r = start[0].cpu().tolist(), np.inf, ref_kw(kw)
    for it in range(n_new):
        if r["e"] >= 0 and it > 0 and cur[-1] == r["e"]:
            cur += [r["e"]] * (n_new - it)
            break
        with torch.no_grad():
            _, logits = g(torch.tensor([cur], device="cuda"), prefix=pf)
        z = rules_ref(logits[0, -1].float().cpu().numpy(), cur, it, **r)
        best = np.sort(z[np.isfinite(z)])[::-1]
        margin = min(margin, float(best[0] - best[1]))
        cur.append(int(np.argmax(z)))
    return cur, margin


def repeated_ngrams(tokens, n):
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) - len(set(grams))


def upto_eos(tokens, t0, e):
    """the sequence up to and including its first generated end-of-text id (the padding behind it repeats that id on purpose)"""
    gen = tokens[t0:]
    return tokens if e not in gen else tokens[:t0 + gen.index(e) + 1]


@pytest.mark.parametrize("name", sorted(MODEL_RULES))
def test_generate_with_the_rules_agrees_on_every_path(golden, fp32_mode, name):  # noqa: F811
    g, zz, start, pf, _ = small_gpt(golden)
    kw = MODEL_RULES[name]
    want, margin = loop_chain(g, start, pf, NEW, **kw)
    print(f"{name}: smallest gap between the two best ruled candidates {margin:.3g}")
    assert margin >= ORDER_MARGIN
    for path in (dict(use_cache=True, use_graph=False), dict(use_cache=True, use_graph=True), dict(use_cache=False)):
        out = g.generate(start.clone(), NEW, prefix=pf, top_k=1, **path, **kw)
        assert out.cpu().tolist() == want, (path, out.cpu().tolist(), want)
    # what the rule promises, and that the call without it does not deliver it (so the rule has reached the paths above)
    plain = g.generate(start.clone(), NEW, prefix=pf, top_k=1, use_cache=True, use_graph=False).cpu().tolist()
    assert plain[:12] == zz["tokens"].tolist()                                                       # the reference's loop: 24 24 24 24 90 208 208 208
    t0, n, m, e = 4, kw.get("no_repeat_ngram_size", 0), kw.get("min_new_tokens", 0), kw.get("eos_token_id", -1)
    if n:
        assert repeated_ngrams(upto_eos(want, t0, e), n) == 0 and repeated_ngrams(plain, n) > 0
    if m:
        assert e not in want[t0:t0 + m] and e in plain[t0:t0 + m]
    if "repetition_penalty" in kw:
        assert want != plain


# =============================================================================================== 5. beam search
def two_sentences():
    cfgo, prefix, tk, idx = C.gpt_small(True)
    return idx[:2, :4].cuda(), prefix[:2].cuda()


@pytest.mark.parametrize("eos", [None, 24], ids=["plain", "eos"])
@pytest.mark.parametrize("S", [1, 2])
def test_beam_search_with_topk_equal_width_is_the_ruled_greedy_chain(golden, fp32_mode, S, eos):  # noqa: F811
    """topk == beam_width: the search collapses to its greedy chain (test_cached_beam_search_with_topk_equal_width_is_the_greedy_chain), so
    with the rules it is generate(top_k=1)'s ruled chain: cached eager, cached hipGraph and the re-forward loop.  With the id, sentence 0
    ends at its seventh token and sentence 1 never does."""
    g = small_gpt(golden)[0]
    starts, pfs = two_sentences()
    W = 3
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    if eos is not None:
        kw.update(min_new_tokens=4, eos_token_id=eos)
    want = [g.generate(starts[s:s + 1].clone(), NEW, prefix=pfs[s:s + 1], top_k=1, use_cache=False, **kw).cpu().tolist() for s in range(S)]
    plain = g.generate(starts[:1].clone(), NEW, prefix=pfs[:1], top_k=1, use_cache=False).cpu().tolist()
    assert want[0] != plain and repeated_ngrams(upto_eos(want[0], 4, -1 if eos is None else eos), 2) == 0
    for path in (dict(use_cache=True, use_graph=False), dict(use_cache=True, use_graph=True), dict(use_cache=False)):
        out = g.generate_beam_search(starts[:S].clone(), NEW, pfs[:S], topk=W, beam_width=W, **path, **kw)
        got = [out.cpu().tolist()] if S == 1 else out.cpu().tolist()
        assert got == want, (path, got, want)


# =============================================================================================== 6. the defaults change nothing
def test_the_defaults_make_no_call_and_move_no_token(golden, fp32_mode, monkeypatch):  # noqa: F811
    g, zz, start, pf, _ = small_gpt(golden)
    from frankenstein_amd import kernels

    def boom(*a, **k):
        raise AssertionError("logit_rules_ called with the rules off")

    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    runs = []
    for patched in (False, True):
        if patched:
            monkeypatch.setattr(kernels, "logit_rules_", boom)
        for extra in ({}, off):
            for path in (dict(use_graph=False), dict(use_graph=True), dict(use_cache=False), dict(use_graph=False, eos_token_id=24)):
                torch.manual_seed(5)
                runs.append(("generate", str(path), g.generate(start.clone(), 8, prefix=pf, top_k=10, **path, **extra).cpu().tolist()))
            for path in (dict(use_graph=False), dict(use_graph=True), dict(use_graph=False, eos_token_id=24)):
                out = g.generate_beam_search(start.clone(), 6, pf, topk=10, beam_width=4, use_cache=True, seeds=[99], **path, **extra)
                runs.append(("beam", str(path), out.cpu().tolist()))
    k = len(runs) // 4
    assert runs[:k] == runs[k:2 * k] == runs[2 * k:3 * k] == runs[3 * k:]
    with pytest.raises(AssertionError, match="rules off"):                                          # and the spy does see a ruled call
        g.generate(start.clone(), 4, prefix=pf, top_k=10, no_repeat_ngram_size=2)


# =============================================================================================== 7. Franky passes them on
def test_franky_passes_the_rules_on(fp32_mode):  # noqa: F811
    fr, x, gcfg = build_franky()
    fr = fr.eval()
    eot, kw = 50256, dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)
    xin = x[0].numpy()
    prefix = fr.brain_model(torch.from_numpy(xin[None]).cuda().float())
    ids = torch.full((1, 1), eot, dtype=torch.long, device="cuda")
    want = fr.llm_model.generate(ids, 9, prefix=prefix, top_k=1, eos_token_id=eot, **kw).cpu().tolist()
    n_gen = int(fr.llm_model.last_lengths[0])
    got = fr.generate(xin, max_new_tokens=9, top_k=1, stop=True, **kw).cpu().tolist()
    assert got == want[:1 + n_gen] and n_gen >= 3 and eot not in got[1:4]
    assert repeated_ngrams(got, 2) == 0
    unruled = fr.generate(xin, max_new_tokens=9, top_k=1, stop=True).cpu().tolist()
    print("Franky greedy:", unruled, "with the rules:", got)
    want_b = fr.llm_model.generate_beam_search(ids, 9, prefix, topk=3, beam_width=3, use_cache=True, eos_token_id=eot, **kw).cpu().tolist()
    n_b = int(fr.llm_model.last_beam_lengths[0])
    got_b = fr.generate_beam(xin, max_new_tokens=9, topk=3, beam_width=3, stop=True, **kw).cpu().tolist()
    assert got_b == want_b[:1 + n_b] and n_b >= 3 and eot not in got_b[1:4] and repeated_ngrams(got_b, 2) == 0
    seen = {}
    for fn in ("generate", "generate_beam_search"):
        orig = getattr(fr.llm_model, fn)
        setattr(fr.llm_model, fn, lambda *a, _o=orig, _f=fn, **k: (seen.__setitem__(_f, k), _o(*a, **k))[1])
    fr.generate(xin, max_new_tokens=4, top_k=1, stop=True, **kw)
    fr.generate_beam(xin, max_new_tokens=4, topk=3, beam_width=3, stop=True, **kw)
    for fn in seen:
        assert {k: seen[fn][k] for k in kw} == kw and seen[fn]["eos_token_id"] == eot, fn
    assert len(seen) == 2
