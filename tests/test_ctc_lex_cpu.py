"""Lexicon-constrained CTC prefix beam search without a GPU: the lexicon (utils/lexicon.py: parsing, the compiled trie against the dict),
the float64 restatement (tests/ctc_lex_ref.py) against a brute-force enumeration of all labellings, the cases of tests/ctc_lex_cases.py
(every make() is the CPU proof that the margin rule holds with no sample left out), and the host side of fk_ctc_beam_search_lex
(refusals before any launch)."""
import numpy as np
import pytest

from frankenstein_amd.utils import lexicon as LX
from frankenstein_amd.utils import ngram as NG
from tests import ctc_lex_cases as XC
from tests import ctc_lex_ref as XR


@pytest.fixture(scope="module")
def built():
    from frankenstein_amd import build
    return build.build(verbose=False)


TEXT = """;;; a comment
HELLO  HH AH L OW
HELLO(2)  HH EH L OW   ;;; a variant
TWO T UW
TOO T UW
TO T UW
TO(2) T AH
"""
PH = {"HH": 2, "AH": 3, "L": 4, "OW": 5, "EH": 6, "T": 7, "UW": 8}


def test_parsing_variants_and_errors(tmp_path):
    lex = LX.Lexicon.from_text(TEXT, PH)
    assert lex.words == ["HELLO", "TWO", "TOO", "TO"] and lex.word_to_id == {"HELLO": 0, "TWO": 1, "TOO": 2, "TO": 3} and len(lex) == 4
    assert lex.pronunciations == {(2, 3, 4, 5): [0], (2, 6, 4, 5): [0], (7, 8): [1, 2, 3], (7, 3): [3]}
    path = tmp_path / "lex.txt"
    path.write_text(TEXT)
    assert LX.Lexicon.from_text(str(path), PH).pronunciations == lex.pronunciations
    with pytest.raises(ValueError, match="line 3: unknown phoneme 'ZZ'"):
        LX.Lexicon.from_text("A AH\n;;; x\nB ZZ AH\n", PH)
    with pytest.raises(ValueError, match="line 1"):
        LX.Lexicon.from_text("A\n", PH)
    with pytest.raises(ValueError):
        LX.Lexicon([("a", ())])
    with pytest.raises(ValueError):
        LX.Lexicon([])


def test_homophone_limit():
    LX.Lexicon([(f"w{i}", (2, 3)) for i in range(8)]).compile()
    with pytest.raises(ValueError, match=r"\(2, 3\)"):
        LX.Lexicon([(f"w{i}", (2, 3)) for i in range(9)]).compile()
    big = LX.zipf_lexicon(120, 6, 0, 1, (1, 2), 0, 0.5)             # 20 pronunciations for 120 words: the generator stops at the limit
    assert max(map(len, big.pronunciations.values())) == LX.MAX_HOMOPHONES


def test_pronounce_text_round_trip():
    lex = LX.Lexicon.from_text(TEXT, PH)
    assert lex.pronounce([0, 3, 1], sep=1) == [2, 3, 4, 5, 1, 7, 8, 1, 7, 8, 1]
    assert lex.pronounce([0, 3], sep=1, trailing_sep=False) == [2, 3, 4, 5, 1, 7, 8] and lex.pronounce([], sep=1) == []
    assert lex.text([0, 3, 1, -100], 3) == "HELLO TO TWO"
    assert lex.text(np.array([[[0, 3, -100]], [[2, -100, -100]]]), np.array([[2], [1]])) == [["HELLO TO"], ["TOO"]]
    prons, prefixes = XR.lexicon_dicts(lex)                         # the labelling spells the transcript back, through the dicts
    lab, part, words = lex.pronounce([0, 1], 1), (), []
    for c in lab:
        if c == 1:
            words.append(prons[part])
            part = ()
        else:
            part += (c,)
            assert part in prefixes
    assert words == [[0], [1, 2, 3]]


@pytest.mark.parametrize("name", ["x", "h", "s", "c", "big"])
def test_compiled_trie_equals_the_dict(name, built):
    """validate(), child / words_at against the dict on every node and every class, the home slots against fk_ngram_hash"""
    from frankenstein_amd import _lib
    lex = XC.lexicon(name)
    t = lex.compile()
    t.validate()
    prons, prefixes = XR.lexicon_dicts(lex)
    assert t.n_nodes == len(prefixes) and t.n_entries == t.n_nodes - 1 and t.cap >= 2 * t.n_entries and t.cap & (t.cap - 1) == 0
    assert t.n_words == len(lex) and sorted(set(t.word_list.tolist())) == list(range(len(lex))) and t is lex.compile()
    classes = sorted({c for p in prons for c in p}) + [0, 1, 1000]
    node = {(): 0}
    for p in sorted(prefixes, key=len):                              # parents first
        n = node[p]
        assert t.words_at(n) == prons.get(p, []), p
        for c in classes:
            ch = t.child(n, c)
            if p + (c,) in prefixes:
                assert ch > 0 and node.setdefault(p + (c,), ch) == ch, (p, c)
            else:
                assert ch == -1, (p, c)
    assert len(set(node.values())) == len(prefixes)
    used = np.nonzero(t.table[:, 0] >= 0)[0]
    for i in used[:200]:
        n, c = int(t.table[i, 0]), int(t.table[i, 1])
        home = _lib.lib().fk_ngram_hash(n, c) & (t.cap - 1)
        assert home == int(NG.hash_slot(n, c, t.cap)) and 0 <= (i - home) & (t.cap - 1) < t.max_probe


def test_validate_refuses_a_broken_table():
    t = XC.lexicon("h").compile()
    for change in (lambda a: a["table"].__setitem__((np.nonzero(a["table"][:, 0] >= 0)[0][0], 2), 99),
                   lambda a: a["node_words"].__setitem__((1, 1), 9), lambda a: a["word_list"].__setitem__(0, 77),
                   lambda a: a["node_words"].__setitem__((0, 1), 1)):
        a = dict(table=t.table.copy(), node_words=t.node_words.copy(), word_list=t.word_list.copy())
        change(a)
        with pytest.raises(ValueError):
            LX.CompiledLexicon(a["table"], a["node_words"], a["word_list"], t.max_probe, t.n_words)
    with pytest.raises(ValueError):
        LX.CompiledLexicon(t.table, t.node_words, t.word_list, 0, t.n_words)


def test_ref_equals_brute_force():
    """case "x", nothing pruned: every labelling the lexicon admits, with its CTC log-probability plus the LM terms, in the same order"""
    case = XC.make("x")
    for b in range(case["logits"].shape[0]):
        x = case["logits"][b, :int(case["input_lengths"][b])].numpy()
        truth = XR.brute_force(x, case["prons"], case["prefixes"], case["lm"], case["blank"], case["sep"], case["lm_weight"], case["word_bonus"])
        truth = {p: v for p, v in truth.items() if np.isfinite(v[0])}
        assert len(truth) > 8 and any(not v[4] for v in truth.values()), b
        hyps, _, _, _ = XR.search_one(x, case["prons"], case["prefixes"], case["lm"], case["blank"], case["sep"], max(32, len(truth)),
                                      x.shape[1] - 1, case["lm_weight"], case["word_bonus"])
        assert [h[0] for h in hyps[:32]] == [h[0] for h in case["ref"]["hyps"][b]]
        assert len(hyps) == len(truth) and {h[0] for h in hyps} == set(truth), b
        for p, am, lm, total, words, done in hyps:
            t = truth[p]
            assert abs(am - t[0]) <= 1e-12 and abs(lm - t[1]) <= 1e-12 and abs(total - t[2]) <= 1e-12 and words == t[3] and done == t[4], (b, p)
        want = sorted(truth, key=lambda p: (not truth[p][4], -truth[p][2]))
        assert [h[0] for h in hyps] == want, b


@pytest.mark.parametrize("key", XC.KEYS)
def test_cases_hold_the_margin_and_their_purpose(key):
    """make() asserts the margin rule for every sample and the mechanism of the table; the result has the declared shapes"""
    case = XC.make(key)
    ref = case["ref"]
    B, T, C = case["logits"].shape
    assert ref["words"].shape == (B, case["nbest"], (T + 1) // 2) and ref["ids"].shape == (B, case["nbest"], T)
    assert np.all(case["e32"] < 1e-3) and np.all(np.isfinite(ref["total"][:, 0]))
    for b in range(B):
        for h, (p, am, lm, total, words, done) in enumerate(ref["hyps"][b][:case["nbest"]]):
            assert XC.admitted(p, case["prons"], case["prefixes"], case["sep"]) and len(words) <= (T + 1) // 2
            assert ref["complete"][b, h] == done and ref["word_lengths"][b, h] == len(words)
        n = len(ref["hyps"][b])
        assert np.all(ref["word_lengths"][b, n:] == 0) and np.all(np.isneginf(ref["total"][b, n:])) and np.all(ref["complete"][b, n:] == 0)
    if key == "p_bf16":
        assert np.array_equal(case["logits"], case["logits"].to(dtype=__import__("torch").bfloat16).float())


def test_planted_logits_spell_the_planted_words():
    """the restatement on the planted case (the GPU test decodes it without the restatement)"""
    pl = XC.planted()
    prons, prefixes = XR.lexicon_dicts(pl["lexicon"])
    ref = XR.beam_search(pl["logits"].numpy(), prons, prefixes, pl["lm"], pl["sep"], pl["input_lengths"].numpy(), pl["blank"], 8, 8, 1, 0.5, 0.0)
    for b, ws in enumerate(pl["words"]):
        assert list(ref["words"][b, 0, :len(ws)]) == ws and ref["word_lengths"][b, 0] == len(ws) and ref["complete"][b, 0] == 1


def test_workspace_and_refusals_need_no_gpu(built):
    """the workspace query, and every refusal of fk_ctc_beam_search_lex returns -1 with its message before any launch"""
    from frankenstein_amd import _lib
    lib = _lib.lib()
    base, mine = lib.fk_ctc_beam_workspace_bytes(2, 32, 8, 12), lib.fk_ctc_beam_lex_workspace_bytes(2, 32, 8, 12)
    assert mine >= base + 2 * (32 * 8 + 1) * 4 and mine % 256 == 0
    assert lib.fk_ctc_beam_lex_workspace_bytes(2, 32, 33, 12) == 0 and lib.fk_ctc_beam_lex_workspace_bytes(0, 32, 8, 12) == 0
    P = 4096                                            # never dereferenced
    big = 1 << 30
    inf, nan = float("inf"), float("nan")

    def run(logits=P, ldb=32 * 41, ldt=41, B=2, T=32, C=41, blank=0, sep=1, W=8, K=12, nbest=4, trie=P, tcap=4096, tprobe=9, node_words=P, nodes=1900,
            word_list=P, n_list=2000, V=2000, table=P, cap=1024, max_probe=3, bow=P, backoff=P, states=100, uni_lp=P, uni_next=P, start=1,
            order=3, weight=1.0, bonus=0.0, words=P, ldwb=4 * 16, ldwh=16, word_lengths=P, ids=P, ldib=4 * 32, ldih=32, lengths=P, am=P, lm=P,
            total=P, complete=P, dtype=_lib.FK_F32, ws=P, nbytes=big):
        return lib.fk_ctc_beam_search_lex(logits, ldb, ldt, None, B, T, C, blank, sep, W, K, nbest, -100, trie, tcap, tprobe, node_words, nodes,
                                          word_list, n_list, V, table, cap, max_probe, bow, backoff, states, uni_lp, uni_next, start, order,
                                          weight, bonus, 1, words, ldwb, ldwh, word_lengths, ids, ldib, ldih, lengths, am, lm, total, complete,
                                          dtype, ws, nbytes, None)

    for kw, msg in [(dict(sep=41), b"sep = 41"), (dict(sep=-1), b"sep = -1"), (dict(sep=0), b"equal to blank"), (dict(trie=None), b"null pointer"),
                    (dict(node_words=None), b"null pointer"), (dict(word_list=None), b"null pointer"), (dict(table=None), b"null pointer"),
                    (dict(bow=None), b"null pointer"), (dict(backoff=None), b"null pointer"), (dict(uni_lp=None), b"null pointer"),
                    (dict(uni_next=None), b"null pointer"), (dict(words=None), b"null pointer"), (dict(word_lengths=None), b"null pointer"),
                    (dict(lm=None), b"null pointer"), (dict(total=None), b"null pointer"), (dict(complete=None), b"null pointer"),
                    (dict(trie=P + 8), b"16-byte aligned"), (dict(table=P + 8), b"16-byte aligned"), (dict(node_words=P + 4), b"8-byte aligned"),
                    (dict(tcap=1000), b"trie cap = 1000"), (dict(tcap=0), b"trie cap = 0"), (dict(tprobe=0), b"trie max_probe = 0"),
                    (dict(tprobe=4097), b"trie max_probe = 4097"), (dict(cap=1000), b"LM cap = 1000"), (dict(max_probe=0), b"LM max_probe = 0"),
                    (dict(max_probe=1025), b"LM max_probe = 1025"), (dict(nodes=0), b"nodes = 0"), (dict(n_list=0), b"word list of 0"),
                    (dict(V=0), b"V = 0"), (dict(order=0), b"order = 0"), (dict(order=9), b"order = 9"), (dict(states=0), b"states = 0"),
                    (dict(start=100), b"start_state = 100"), (dict(weight=inf), b"must be finite"), (dict(weight=nan), b"must be finite"),
                    (dict(bonus=-inf), b"must be finite"), (dict(bonus=nan), b"must be finite"), (dict(ldwh=15), b"words strides"),
                    (dict(ldwb=3 * 16 + 15), b"words strides"), (dict(ws=None), b"workspace too small"),
                    (dict(nbytes=lib.fk_ctc_beam_lex_workspace_bytes(2, 32, 8, 12) - 1), b"workspace too small"),
                    (dict(nbytes=lib.fk_ctc_beam_workspace_bytes(2, 32, 8, 12)), b"workspace too small"),
                    # and everything fk_ctc_beam_search refuses, under this entry's name
                    (dict(logits=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(lengths=None), b"null pointer"),
                    (dict(am=None), b"null pointer"), (dict(dtype=7), b"dtype"), (dict(B=0), b"B = 0"), (dict(T=0), b"T = 0"), (dict(C=1), b"C = 1"),
                    (dict(blank=41), b"blank = 41"), (dict(W=0), b"envelope"), (dict(W=33), b"envelope"), (dict(K=0), b"envelope"),
                    (dict(K=33), b"envelope"), (dict(nbest=0), b"nbest = 0"), (dict(nbest=9), b"nbest = 9"), (dict(ldt=40), b"row stride 40 below C"),
                    (dict(ldih=31), b"ids strides"), (dict(ldib=3 * 32 + 31), b"ids strides")]:
        assert run(**kw) == -1 and msg in lib.fk_last_error() and b"fk_ctc_beam_search_lex" in lib.fk_last_error(), (kw, lib.fk_last_error())


def test_word_model_must_match_the_lexicon():
    """a word model over another vocabulary raises before anything touches a device"""
    import torch
    from frankenstein_amd import kernels as K
    lex = XC.lexicon("h")
    with pytest.raises(ValueError, match="the word model has 4 words, the lexicon 6"):
        K.ctc_beam_search_lex(torch.zeros(1, 4, 5), lex, XC.model("x"), sep=1)
    with pytest.raises(ValueError, match="a pronunciation holds"):
        K.ctc_beam_search_lex(torch.zeros(1, 4, 5), lex, XC.model("h"), sep=2)
    with pytest.raises(ValueError, match="a pronunciation holds"):
        K.ctc_beam_search_lex(torch.zeros(1, 4, 4), lex, XC.model("h"), sep=1)
