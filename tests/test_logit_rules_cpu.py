"""CPU-side checks of the rules that depend on the tokens already emitted (repetition penalty, n-gram ban, minimum length): the torch
restatement GPT._apply_logit_rules against the loop-by-loop `rules_ref` written here, bit for bit; fk_logit_rules is exported, bound and
refuses what lies outside its envelope on the host; the public entry points refuse bad arguments before any GPU work.

`rules_ref` is the rule of include/franken_hip.h (fk_logit_rules) with nothing but Python loops and numpy float32 scalars;
tests/test_logit_rules_gpu.py holds the kernel and every decode path to it."""
import ctypes
import math

import numpy as np
import pytest
import torch

EINVAL = -1
P = 16                # a non-null "pointer": the argument checks come before any GPU call and never follow it
NEG = -np.inf


def rules_ref(z, h, g, p=1.0, n=0, m=0, e=-1):
    """One row.  z fp32 [V], h the history (prompt ids, then the generated tokens), g generated tokens, e the end-of-text id or -1."""
    z = np.asarray(z, np.float32)
    V, L, h = len(z), len(h), [int(v) for v in h]
    out = z.copy()
    pf = np.float32(p)
    inv = np.float32(1.0 / np.float64(pf))                 # float64 quotient, rounded once
    seen = set()
    for v in h:                                            # 1. every distinct in-range token but e, once, from the ORIGINAL logit
        if 0 <= v < V and v != e and v not in seen:
            seen.add(v)
            out[v] = np.float32(z[v] * inv) if z[v] > 0 else np.float32(z[v] * pf)
    if n >= 1 and L >= n:                                  # 2. what followed the last n - 1 tokens before may not follow them again
        for j in range(L - n + 1):
            if h[j:j + n - 1] == h[L - n + 1:]:
                v = h[j + n - 1]
                if 0 <= v < V and v != e:
                    out[v] = NEG
    if g < m and 0 <= e < V:                               # 3. not yet
        out[e] = NEG
    return out


def apply(z, h, g, p=1.0, n=0, m=0, e=-1):
    from frankenstein_amd.models.gpt2_model import GPT
    zz = torch.from_numpy(np.asarray(z, np.float32))[None].clone()
    before = zz.clone()
    got = GPT._apply_logit_rules(zz, torch.tensor([list(h)], dtype=torch.long).view(1, len(h)), g, repetition_penalty=p, no_repeat_ngram_size=n,
                                 min_new_tokens=m, eos_token_id=None if e < 0 else e)
    assert torch.equal(zz.view(torch.int32), before.view(torch.int32))                         # the input is never written (bits: a NaN too)
    return got[0]


V0 = 12
# positive, negative and zero logits (both signs of zero); token 0 and token V - 1 carry values whose sign matters
Z0 = np.array([2.5, -1.25, 0.0, 3.0, -0.0, 0.7, -4.0, 1e-3, -7.5, 0.3333, 5.0, -2.0], np.float32)


def same(got, want):
    return torch.equal(got, torch.from_numpy(want)) and got.dtype == torch.float32


@pytest.mark.parametrize("p", [1.3, 0.8])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_restatement_at_every_history_length_around_n(n, p):
    """L in {0, 1, n - 1, n, n + 1}: below n nothing is banned; the histories hold token 0 and token V - 1"""
    base = [0, V0 - 1, 0, V0 - 1, 3]
    for L in sorted({0, 1, n - 1, n, n + 1}):
        h = base[:L]
        want = rules_ref(Z0, h, 0, p, n, 0, -1)
        assert same(apply(Z0, h, 0, p, n, 0, -1), want), (L, h)
        if L < n:
            assert not np.isinf(want).any()
        alone = rules_ref(Z0, h, 0, 1.0, n, 0, -1)
        assert same(apply(Z0, h, 0, 1.0, n, 0, -1), alone)
        assert np.array_equal(alone[np.isfinite(alone)], Z0[np.isfinite(alone)])


@pytest.mark.parametrize("p", [1.3, 0.8])
def test_restatement_on_the_crafted_histories(p):
    pf = np.float32(p)
    inv = np.float32(1.0 / np.float64(pf))
    # the same token three times: penalised once, from the original logit
    want = rules_ref(Z0, [3, 5, 3, 6, 3], 2, p)
    assert want[3] == np.float32(Z0[3] * inv) and want[6] == np.float32(Z0[6] * pf) and want[5] == np.float32(Z0[5] * inv)
    assert same(apply(Z0, [3, 5, 3, 6, 3], 2, p), want)
    # zero logits (both signs) take the `z * p` side and stay zero; an unseen token keeps its logit
    want = rules_ref(Z0, [2, 4], 0, p)
    assert want[2] == 0.0 and want[4] == 0.0 and np.signbit(want[4]) and want[1] == Z0[1]
    assert same(apply(Z0, [2, 4], 0, p), want)
    # the same (n - 1)-gram followed by two different tokens: both banned; token 1 is seen AND banned: -inf wins
    for n, h in ((2, [7, 1, 9, 7, 8, 7]), (3, [7, 7, 1, 5, 7, 7, 8, 7, 7])):
        want = rules_ref(Z0, h, 0, p, n)
        assert want[1] == NEG and want[8] == NEG and np.isinf(want).sum() == 2
        assert want[7] == np.float32(Z0[7] * inv)              # seen, not banned
        assert same(apply(Z0, h, 0, p, n), want), n
    # overlapping windows: h = a a a with n = 3 bans a (j = 0: (a, a) is followed by a)
    want = rules_ref(Z0, [5, 5, 5], 0, 1.0, 3)
    assert want[5] == NEG and same(apply(Z0, [5, 5, 5], 0, 1.0, 3), want)
    # token 0 and token V - 1, ids -1 and V (ignored, also as the banned follower and inside the compared (n-1)-gram)
    h = [-1, V0, 0, V0 - 1, -1, V0, 0, -1]
    for n in (0, 1, 2, 3):
        want = rules_ref(Z0, h, 0, p, n)
        assert same(apply(Z0, h, 0, p, n), want), n
    assert not np.isinf(rules_ref(Z0, h, 0, p, 2)).any()       # the last token, -1, was only ever followed by V: nothing to ban
    want = rules_ref(Z0, [0, V0 - 1, 4, 0], 0, p, 2)
    assert want[V0 - 1] == NEG and want[0] == np.float32(Z0[0] * inv) and same(apply(Z0, [0, V0 - 1, 4, 0], 0, p, 2), want)


@pytest.mark.parametrize("p", [1.3, 0.8])
def test_the_end_of_text_id_is_exempt_from_the_penalty_and_the_ban(p):
    e = 10
    h = [e, 3, e, 3, e]                                        # e seen three times
    for n, h in ((1, h), (2, h[:4])):                          # n = 2: the last token, 3, was followed by e before
        want = rules_ref(Z0, h, 5, p, n, 0, e)
        assert want[e] == Z0[e] and (want[3] == NEG) == (n == 1)
        assert same(apply(Z0, h, 5, p, n, 0, e), want)
        other = rules_ref(Z0, h, 5, p, n, 0, -1)               # without an id it is a token like any other
        assert other[e] == NEG and same(apply(Z0, h, 5, p, n, 0, -1), other)
    assert rules_ref(Z0, h, 5, p, 0, 0, -1)[e] == np.float32(Z0[e] * np.float32(1.0 / np.float64(np.float32(p))))       # and penalised
    h = [e, 3, e, 3, e]
    # minimum length: g = m - 1 masks, g = m does not; the mask is the only thing that ever touches z[e]
    for g, masked in ((0, True), (3, True), (4, False), (9, False)):
        want = rules_ref(Z0, h, g, p, 2, 4, e)
        assert (want[e] == NEG) == masked and (masked or want[e] == Z0[e])
        assert same(apply(Z0, h, g, p, 2, 4, e), want), g
    want = rules_ref(Z0, [], 0, 1.0, 0, 1, e)                   # the minimum length alone, empty history
    assert np.isinf(want).sum() == 1 and want[e] == NEG and same(apply(Z0, [], 0, 1.0, 0, 1, e), want)


def test_restatement_on_random_rows_and_batches():
    """random histories over a small vocabulary (many repeats), every combination of the three rules, as ONE batched call"""
    from frankenstein_amd.models.gpt2_model import GPT
    rng = np.random.default_rng(5)
    B, V, L = 16, 9, 14
    z = rng.standard_normal((B, V)).astype(np.float32) * 3
    h = rng.integers(-1, V + 1, (B, L))
    for p in (1.0, 1.3, 0.8):
        for n in (0, 1, 2, 3, 4):
            for m, e in ((0, -1), (0, 4), (3, 4)):
                got = GPT._apply_logit_rules(torch.from_numpy(z), torch.from_numpy(h), 2, repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m,
                                             eos_token_id=None if e < 0 else e)
                want = np.stack([rules_ref(z[b], h[b], 2, p, n, m, e) for b in range(B)])
                assert torch.equal(got, torch.from_numpy(want)), (p, n, m, e)


def test_nan_logits_stay_nan():
    z = Z0.copy()
    z[3] = np.nan
    got = apply(z, [3, 5], 0, 1.3, 0, 0, -1)
    assert math.isnan(float(got[3])) and float(got[5]) == float(np.float32(Z0[5] * np.float32(1.0 / np.float64(np.float32(1.3)))))


def test_defaults_return_the_input_unchanged():
    from frankenstein_amd.models.gpt2_model import GPT
    z = torch.from_numpy(Z0)[None].clone()
    h = torch.tensor([[3, 3, 5]])
    assert GPT._apply_logit_rules(z, h, 0) is z
    assert GPT._apply_logit_rules(z, h, 0, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, eos_token_id=4) is z
    assert torch.equal(z[0], torch.from_numpy(Z0))


def test_host_sample_with_top_k_1_is_the_argmax_of_the_restated_row():
    from frankenstein_amd.models.gpt2_model import GPT
    rng = np.random.default_rng(8)
    z = (rng.standard_normal((6, 40)) * 2).astype(np.float32)
    h = np.stack([np.argsort(-z[b])[[1, 0, 2, 1]] for b in range(6)])                  # the best token is seen, and it has followed the last one
    for kw, ref in ((dict(no_repeat_ngram_size=1), dict(n=1)), (dict(no_repeat_ngram_size=2), dict(n=2)), (dict(repetition_penalty=50.0), dict(p=50.0)),
                    (dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, eos_token_id=int(np.argsort(-z[0])[3])),
                     dict(p=1.3, n=2, m=3, e=int(np.argsort(-z[0])[3])))):
        want = [int(np.argmax(rules_ref(z[b], h[b], 1, **ref))) for b in range(6)]
        rules = GPT._check_logit_rules(kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), kw.get("min_new_tokens", 0), kw.get("eos_token_id"), 40, 5, 1)
        got = GPT._sample(torch.from_numpy(z), 1.0, 1, rules=rules, history=torch.from_numpy(h), generated=1).view(-1).tolist()
        assert got == want, kw
        assert got != np.argmax(z, -1).tolist()
    assert GPT._sample(torch.from_numpy(z), 1.0, 1, history=torch.from_numpy(h), generated=1).view(-1).tolist() == np.argmax(z, -1).tolist()


# =============================================================================================== the export
@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_export_exists(lib):
    from frankenstein_amd import _lib
    from frankenstein_amd import kernels as K
    h = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(h, "fk_logit_rules") and "fk_logit_rules" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["fk_logit_rules"][1]) == 20
    assert callable(K.logit_rules_) and K.LogitRules is not None
    assert K.inv_penalty(1.3) == (float(np.float32(1.3)), float(np.float32(1.0 / np.float64(np.float32(1.3)))))


def rules(lib, logits=P, ld=216, R=6, V=211, penalty=1.3, ngram=2, min_new=1, eos=7, step=P, cur=P, hist=P, hist2=None, hist_ld=12, t0=4, steps=8,
          parent_log=None, log_rows=0, W=0, broadcast=0):
    return lib.fk_logit_rules(logits, ld, R, V, penalty, ngram, min_new, eos, step, cur, hist, hist2, hist_ld, t0, steps, parent_log, log_rows, W, broadcast, None)


BEAM = dict(hist2=P, parent_log=P, log_rows=8, W=3)


@pytest.mark.parametrize("mode", [{}, BEAM], ids=["plain", "beam"])
def test_logit_rules_refuses_bad_arguments(lib, mode):
    for name in ("logits", "step", "cur", "hist"):
        assert rules(lib, **{**mode, name: None}) == EINVAL and b"fk_logit_rules: null pointer" in lib.fk_last_error(), name
    for kw in (dict(R=0), dict(R=65536 * 3), dict(V=0), dict(V=1 << 31, ld=1 << 31), dict(ld=210)):
        assert rules(lib, **{**mode, **kw}) == EINVAL and b"fk_logit_rules: bad arguments" in lib.fk_last_error(), kw
    for p in (0.0, -1.3, math.nan, math.inf, -math.inf):
        assert rules(lib, penalty=p, **mode) == EINVAL and b"fk_logit_rules: need a finite penalty > 0" in lib.fk_last_error(), p
    for kw in (dict(ngram=-1), dict(min_new=-1), dict(eos=1 << 31)):
        assert rules(lib, **{**mode, **kw}) == EINVAL and b"fk_logit_rules: need 0 <= ngram" in lib.fk_last_error(), kw
    for kw in (dict(hist_ld=11), dict(t0=-1), dict(steps=-1), dict(t0=4000, steps=97, hist_ld=5000)):
        assert rules(lib, **{**mode, **kw}) == EINVAL and b"fk_logit_rules: a history row holds" in lib.fk_last_error(), kw


def test_logit_rules_refuses_a_bad_beam_mode(lib):
    assert rules(lib, hist2=P) == EINVAL and b"both or none" in lib.fk_last_error()
    assert rules(lib, parent_log=P, log_rows=8, W=3) == EINVAL and b"both or none" in lib.fk_last_error()
    for W in (0, -1, 17):
        assert rules(lib, **{**BEAM, "W": W}) == EINVAL and b"fk_logit_rules: need 1 <= W <= 16" in lib.fk_last_error(), W
    assert rules(lib, **{**BEAM, "log_rows": -1}) == EINVAL and b"log_rows" in lib.fk_last_error()
    assert rules(lib, R=7, **BEAM) == EINVAL and b"S sentences x W beams" in lib.fk_last_error()          # 7 rows are no multiple of 3 beams
    assert rules(lib, R=40000, broadcast=1, **BEAM) == EINVAL and b"S sentences x W beams" in lib.fk_last_error()
    assert rules(lib, broadcast=1) == EINVAL and b"broadcast belongs to the beam mode" in lib.fk_last_error()


# =============================================================================================== the public entry points
def tiny():
    from frankenstein_amd.models.gpt2_model import GPT, GPTConfig
    return GPT(GPTConfig(block_size=16, vocab_size=32, n_layer=1, n_head=2, n_embd=16, dropout=0.0, bias=True))


BAD = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=math.nan), dict(repetition_penalty=math.inf),
       dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(no_repeat_ngram_size=2.0), dict(min_new_tokens=-2), dict(min_new_tokens=0.5)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_entry_points_refuse_bad_rule_arguments(bad):
    from frankenstein_amd.models.notebook_models import Franky
    g = tiny()
    name = next(iter(bad))
    ids = torch.zeros((1, 1), dtype=torch.long)
    kw = dict(bad, eos_token_id=3) if name == "min_new_tokens" else bad
    with pytest.raises(ValueError, match=name):
        g.generate(ids, 2, **kw)
    with pytest.raises(ValueError, match=name):
        g.generate(ids, 2, **{**kw, "eos_token_id": 3})
    with pytest.raises(ValueError, match=name):
        g.generate_beam_search(ids, 2, None, topk=4, beam_width=2, **kw)
    with pytest.raises(ValueError, match=name):
        g.generate_beam_search(ids, 2, None, topk=4, beam_width=2, use_cache=True, **{**kw, "eos_token_id": 3})
    fr = Franky(torch.nn.Identity(), g)
    x = np.zeros((4, 2), np.float32)
    for stop in (False, True):
        if name == "min_new_tokens" and not stop:
            continue
        with pytest.raises(ValueError, match=name):
            fr.generate(x, 2, stop=stop, **bad)
        with pytest.raises(ValueError, match=name):
            fr.generate_beam(x, 2, topk=4, beam_width=2, stop=stop, **bad)


def test_min_new_tokens_needs_an_end_of_text_id():
    from frankenstein_amd.models.notebook_models import Franky
    g = tiny()
    ids = torch.zeros((1, 1), dtype=torch.long)
    with pytest.raises(ValueError, match="min_new_tokens needs an eos_token_id"):
        g.generate(ids, 2, min_new_tokens=1)
    with pytest.raises(ValueError, match="min_new_tokens needs an eos_token_id"):
        g.generate_beam_search(ids, 2, None, topk=4, beam_width=2, min_new_tokens=1)
    fr = Franky(torch.nn.Identity(), g)                        # stop=False: no end-of-text id reaches the decoder
    with pytest.raises(ValueError, match="min_new_tokens needs an eos_token_id"):
        fr.generate(np.zeros((4, 2), np.float32), 2, min_new_tokens=1)
    with pytest.raises(ValueError, match="min_new_tokens needs an eos_token_id"):
        fr.generate_beam(np.zeros((4, 2), np.float32), 2, topk=4, beam_width=2, min_new_tokens=1)


def test_the_vocabulary_must_outlast_the_rules():
    """V = 32: the rules may remove total_len + 1 tokens, and max(top_k, 1) candidates must be left"""
    g = tiny()
    ids = torch.zeros((1, 3), dtype=torch.long)                # total_len = 3 + 8 = 11: 32 - 12 = 20 candidates are left for certain
    with pytest.raises(ValueError, match="candidates"):
        g.generate(ids, 8, top_k=21, no_repeat_ngram_size=1)
    with pytest.raises(ValueError, match="candidates"):
        g.generate_beam_search(ids, 8, None, topk=21, beam_width=2, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="candidates"):
        g.generate(torch.zeros((1, 3), dtype=torch.long), 28, no_repeat_ngram_size=1)        # 32 - 32 < 1
    assert g._check_logit_rules(1.2, 1, 0, None, 32, 11, 20) is not None                      # exactly enough
    assert g._check_logit_rules(1.0, 0, 0, None, 32, 1000, 20) is None                        # all off: nothing to check
