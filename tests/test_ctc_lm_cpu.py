"""N-gram shallow fusion in the CTC prefix beam search without a GPU: the language model (utils/ngram.py: estimation, the ARPA parser, the
compiled state machine against the dictionary definition), the float64 restatement (tests/ctc_lm_ref.py) against a brute-force enumeration
and against the plain search, the cases of tests/ctc_lm_cases.py, and the host side of fk_ctc_beam_search_lm (refusals before any launch)."""
import itertools
import math

import numpy as np
import pytest

from frankenstein_amd.utils import ngram as NG
from tests import ctc_beam_ref as BR
from tests import ctc_lm_cases as LC
from tests import ctc_lm_ref as LR

ALL = sorted(LC.CASES) + ["v_bf16", "e_noeos"]


@pytest.fixture(scope="module")
def built():
    from frankenstein_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def small():
    """3 tokens (class 2 never occurs: it stands for a blank), order 3"""
    return NG.NGramLM.from_corpus(NG.zipf_sequences(30, 3, 2, (1, 5), 1), 3, 3)


def contexts(lm, longest):
    """every history of up to `longest` class ids, with and without the start of sentence in front: seen and unseen alike"""
    for n in range(longest + 1):
        for ctx in itertools.product(range(lm.n_classes), repeat=n):
            yield ctx
            yield (lm.bos,) + ctx


def test_witten_bell_sums_to_one(small):
    assert small.start_context == (small.bos,)
    for ctx in contexts(small, 3):
        total = sum(math.exp(small.score(ctx, c)) for c in range(small.n_classes + 1))
        assert abs(total - 1.0) <= 1e-14, (ctx, total)
    # a listed n-gram is the interpolated estimate itself
    seqs = NG.zipf_sequences(30, 3, 2, (1, 5), 1)
    first = [s[0] for s in seqs]
    n, t = len(first), len(set(first))
    c = first[0]
    uni = math.exp(small.score((), c))
    assert abs(math.exp(small.score((small.bos,), c)) - (first.count(c) + t * uni) / (n + t)) <= 1e-15


def test_compiled_lookup_equals_score(small, built):
    from frankenstein_amd import _lib
    t = small.compile()
    assert t.n_states > 3 and t.cap >= 2 * t.n_entries and t.cap & (t.cap - 1) == 0 and t.start_state == small.state_of((small.bos,)) != 0
    for s, c in ((1, 2), (12345, 50257), (2 ** 31 - 1, 7)):            # the hash of the header, as the library computes it
        assert _lib.lib().fk_ngram_hash(s, c) & 1023 == int(NG.hash_slot(s, c, 1024))
    for lm in (small, LC.model("b"), LC.model("s")):
        t = lm.compile()
        for ctx in contexts(lm, lm.order if lm.n_classes <= 3 else 2):
            s = lm.state_of(ctx)
            for c in range(lm.n_classes + 1):
                want = lm.score(ctx, c)
                got, nxt = t.lookup(s, c)
                assert abs(got - want) <= 2.0 ** -22 * max(1.0, abs(want)), (ctx, c, got, want)
                if c != lm.eos:
                    assert nxt == lm.state_of(ctx + (c,)), (ctx, c)
    big = LC.model("v").compile()                                        # a table where look-ups meet other entries on their way
    assert big.max_probe > 1 and big.n_entries > 10000
    lm = LC.model("v")
    for g in list(lm.ngrams)[::997]:
        got, _ = big.lookup(lm.state_of(g[:-1]), g[-1])
        assert abs(got - lm.ngrams[g]) <= 2.0 ** -22 * max(1.0, abs(lm.ngrams[g])), g


def test_arpa_round_trip(small, tmp_path):
    names = {0: "a", 1: "b", 2: "c"}
    words = dict(names)
    words[small.eos], words[small.bos] = "</s>", "<s>"
    levels = [[] for _ in range(small.order)]
    for g, lp in small.ngrams.items():
        levels[len(g) - 1].append((g, lp))
    levels[0].append(((small.bos,), -99.0 * NG.LN10))
    lines = ["\\data\\"] + [f"ngram {k + 1}={len(level)}" for k, level in enumerate(levels)]
    for k, level in enumerate(levels):
        lines += ["", f"\\{k + 1}-grams:"]
        for g, lp in sorted(level):
            bow = small.bows.get(g)
            lines.append(f"{lp / NG.LN10!r}\t{' '.join(words[w] for w in g)}" + ("" if bow is None else f"\t{bow / NG.LN10!r}"))
    text = "\n".join(lines + ["", "\\end\\", ""])
    path = tmp_path / "small.arpa"
    path.write_text(text)
    ids = {v: k for k, v in names.items()}
    for src in (text, str(path), small.to_arpa(names)):
        lm = NG.NGramLM.from_arpa(src, ids, 3)
        assert lm.order == small.order and set(lm.ngrams) == set(small.ngrams) and set(lm.bows) == set(small.bows)
        for ctx in contexts(small, 3):
            for c in range(4):
                assert abs(lm.score(ctx, c) - small.score(ctx, c)) <= 1e-13, (ctx, c)
    # a class without a unigram takes <unk>'s value, or unk_logp; without either the file is refused
    short = "\\data\\\nngram 1=3\n\n\\1-grams:\n-0.5\ta\n-0.7\t</s>\n-99\t<s>\t-0.1\n\n\\end\\\n"
    with pytest.raises(ValueError, match="unk_logp"):
        NG.NGramLM.from_arpa(short, ids, 3)
    lm = NG.NGramLM.from_arpa(short, ids, 3, unk_logp=-7.0)
    assert lm.score((), 1) == -7.0 and abs(lm.score((), 0) + 0.5 * NG.LN10) < 1e-15 and lm.bows[(lm.bos,)] == -0.1 * NG.LN10
    lm = NG.NGramLM.from_arpa(short.replace("ngram 1=3", "ngram 1=4").replace("-0.5\ta\n", "-0.5\ta\n-3\t<unk>\n"), ids, 3)
    assert abs(lm.score((), 2) + 3.0 * NG.LN10) < 1e-15


def test_compile_rejects_bad_tables(small):
    t = small.compile()
    parts = dict(table=t.table, bow=t.bow, backoff=t.backoff, uni_lp=t.uni_lp, uni_next=t.uni_next, depth=t.depth, max_probe=t.max_probe,
                 start_state=t.start_state, order=t.order, n_classes=t.n_classes)
    NG.CompiledNGram(**parts)
    deep = int(np.argmax(t.depth))
    same = next(s for s in range(1, t.n_states) if t.depth[s] == t.depth[deep])
    bad = t.backoff.copy()
    bad[deep] = same                                                     # a backoff that does not shorten the context: a loop on the device
    with pytest.raises(ValueError, match="strictly shorter"):
        NG.CompiledNGram(**{**parts, "backoff": bad})
    with pytest.raises(ValueError, match="max_probe"):
        NG.CompiledNGram(**{**parts, "max_probe": 0})
    if t.max_probe > 1:
        with pytest.raises(ValueError, match="beyond max_probe"):
            NG.CompiledNGram(**{**parts, "max_probe": t.max_probe - 1})
    with pytest.raises(ValueError, match="power of two"):
        NG.CompiledNGram(**{**parts, "table": t.table[:-1]})
    nxt = t.table.copy()
    nxt[np.nonzero(nxt[:, 0] >= 0)[0][0], 3] = t.n_states
    with pytest.raises(ValueError, match="next state"):
        NG.CompiledNGram(**{**parts, "table": nxt})
    # a model that is not closed under prefixes: the context (0, 1) occurs, the bigram "0 1" does not
    uni = {(c,): math.log(0.25) for c in range(4)}
    with pytest.raises(ValueError, match="closed under prefixes"):
        NG.NGramLM({**uni, (0, 1, 0): -1.0}, {}, 3, 3).compile()


def test_ref_equals_brute_force():
    """case x, nothing pruned: the same labellings in the same order, am, lm and total within 1e-12 of the enumeration"""
    case = LC.make("x")
    lm, lw, bonus = case["lm"], case["lm_weight"], case["length_bonus"]
    for use_eos in (True, False):
        for b in range(case["logits"].shape[0]):
            x = case["logits"][b, :int(case["input_lengths"][b])].numpy()
            truth = {p: v for p, v in LR.brute_force(x, lm, case["blank"], lw, bonus, use_eos).items() if np.isfinite(v[0])}
            hyps, _, _ = LR.search_one(x, lm, case["blank"], max(32, len(truth)), x.shape[1] - 1, lw, bonus, use_eos)
            assert len(hyps) == len(truth) and {r[0] for r in hyps} == set(truth)
            for p, am, lms, tot in hyps:
                assert max(abs(am - truth[p][0]), abs(lms - truth[p][1]), abs(tot - truth[p][2])) <= 1e-12, (p, am, lms, tot, truth[p])
            assert [r[0] for r in hyps] == sorted(truth, key=lambda p: -truth[p][2])
    ref = case["ref"]                                                    # and the case's own result (W = 32 holds every labelling)
    truth = LR.brute_force(case["logits"][0].numpy(), lm, case["blank"], lw, bonus, True)
    assert [r[0] for r in ref["hyps"][0]] == sorted(truth, key=lambda p: -truth[p][2])


@pytest.mark.parametrize("key", ["s", "b", "r", "m", "t"])
def test_zero_weight_is_the_plain_search(key):
    """lm_weight = 0, length_bonus = 0, no end of sentence: the plain restatement's prefixes, order, gaps, ties and scores, exactly"""
    case = LC.make(key)
    x, il = case["logits"].numpy(), case["input_lengths"].numpy()
    for dtype in (np.float64, np.float32):
        got = LR.beam_search(x, case["lm"], il, case["blank"], case["W"], case["K"], case["nbest"], 0.0, 0.0, False, LC.PAD, dtype)
        want = BR.beam_search(x, il, case["blank"], case["W"], case["K"], case["nbest"], LC.PAD, dtype)
        assert np.array_equal(got["ids"], want["ids"]) and np.array_equal(got["lengths"], want["lengths"])
        assert np.array_equal(got["am"], want["scores"]) and np.array_equal(got["total"], want["scores"])
        assert got["ties"] == want["ties"] and np.array_equal(got["frame_gap"], want["frame_gap"])
        assert [[r[0] for r in h] for h in got["hyps"]] == [[p for p, _ in h] for h in want["hyps"]]


@pytest.mark.parametrize("key", ALL)
def test_cases_keep_their_purpose(key):
    """make() asserts the margin and what the table says the case is for; here: the forms, and that the language model matters"""
    case = LC.make(key)
    ref = case["ref"]
    B, nbest, T = ref["ids"].shape
    have = np.isfinite(ref["total"])
    assert np.all(ref["lengths"][~have] == 0) and np.all(ref["ids"][~have] == LC.PAD) and np.all(np.isneginf(ref["am"][~have])) and np.all(np.isneginf(ref["lm"][~have]))
    with np.errstate(invalid="ignore"):                                  # (-inf - -inf behind the last hypothesis)
        assert have[:, 0].all() and np.all(np.diff(ref["total"], axis=1)[have[:, 1:]] <= 0)
    if key in ("s", "e"):
        eos = case["lm"].score(case["lm"].start_context, case["lm"].eos)
        assert int(case["input_lengths"][2]) == 0 and ref["lengths"][2, 0] == 0 and ref["am"][2, 0] == 0.0 and ref["lm"][2, 0] == eos
        assert np.isneginf(ref["total"][2, 1])
    if key == "e_noeos":
        assert ref["lm"][2, 0] == 0.0 and ref["total"][2, 0] == 0.0
    if key in ("s", "m", "t", "l", "p"):                                 # the fused search does not return the plain search's list
        plain = BR.beam_search(case["logits"].numpy(), case["input_lengths"].numpy(), case["blank"], case["W"], case["K"], case["nbest"], LC.PAD)
        assert not np.array_equal(plain["ids"], ref["ids"]), key
    if key == "t":
        assert ref["frame_gap"].max() < np.inf                            # the table really overflows W = 32
    if key == "l":
        assert ref["lengths"][:, 0].min() > 20
    if key == "v_bf16":
        assert len(ref["ties"][0]) > 0


def test_refusals_need_no_gpu(built):
    """every refusal of fk_ctc_beam_search_lm returns -1 with its message before any launch"""
    from frankenstein_amd import _lib
    lib = _lib.lib()
    P = 4096                                            # never dereferenced
    big = 1 << 30
    inf, nan = float("inf"), float("nan")

    def run(logits=P, ldb=32 * 41, ldt=41, B=2, T=32, C=41, blank=0, W=8, K=12, nbest=4, table=P, cap=1024, max_probe=3, bow=P, backoff=P,
            states=100, uni_lp=P, uni_next=P, start=1, order=3, weight=1.0, bonus=0.0, ids=P, ldib=4 * 32, ldih=32, lengths=P, am=P, lm=P,
            total=P, dtype=_lib.FK_F32, ws=P, nbytes=big):
        return lib.fk_ctc_beam_search_lm(logits, ldb, ldt, None, B, T, C, blank, W, K, nbest, -100, table, cap, max_probe, bow, backoff, states,
                                         uni_lp, uni_next, start, order, weight, bonus, 1, ids, ldib, ldih, lengths, am, lm, total, dtype, ws,
                                         nbytes, None)

    for kw, msg in [(dict(table=None), b"null pointer"), (dict(bow=None), b"null pointer"), (dict(backoff=None), b"null pointer"),
                    (dict(uni_lp=None), b"null pointer"), (dict(uni_next=None), b"null pointer"), (dict(lm=None), b"null pointer"),
                    (dict(total=None), b"null pointer"), (dict(table=P + 8), b"16-byte aligned"), (dict(order=0), b"order = 0"),
                    (dict(order=9), b"order = 9"), (dict(cap=1000), b"cap = 1000"), (dict(cap=0), b"cap = 0"), (dict(max_probe=0), b"max_probe = 0"),
                    (dict(max_probe=1025), b"max_probe = 1025"), (dict(states=0), b"states = 0"), (dict(start=100), b"start_state = 100"),
                    (dict(start=-1), b"start_state = -1"), (dict(weight=inf), b"must be finite"), (dict(weight=nan), b"must be finite"),
                    (dict(bonus=-inf), b"must be finite"), (dict(bonus=nan), b"must be finite"),
                    # and everything fk_ctc_beam_search refuses, under this entry's name
                    (dict(logits=None), b"fk_ctc_beam_search_lm: null pointer"), (dict(ids=None), b"null pointer"), (dict(lengths=None), b"null pointer"),
                    (dict(am=None), b"null pointer"), (dict(ws=None), b"workspace too small"), (dict(dtype=7), b"dtype"), (dict(B=0), b"B = 0"),
                    (dict(T=0), b"T = 0"), (dict(C=1), b"C = 1"), (dict(blank=41), b"blank = 41"), (dict(blank=-1), b"blank = -1"),
                    (dict(W=0), b"envelope"), (dict(W=33), b"envelope"), (dict(K=0), b"envelope"), (dict(K=33), b"envelope"),
                    (dict(nbest=0), b"nbest = 0"), (dict(nbest=9), b"nbest = 9"), (dict(ldt=40), b"row stride 40 below C"), (dict(ldb=40), b"row stride"),
                    (dict(ldih=31), b"ids strides"), (dict(ldib=3 * 32 + 31), b"ids strides"),
                    (dict(nbytes=lib.fk_ctc_beam_workspace_bytes(2, 32, 8, 12) - 1), b"workspace too small")]:
        assert run(**kw) == -1 and msg in lib.fk_last_error() and b"fk_ctc_beam_search_lm" in lib.fk_last_error(), (kw, lib.fk_last_error())
