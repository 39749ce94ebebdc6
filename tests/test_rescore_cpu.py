"""LM rescoring of n-best lists without a GPU: the float64 restatement (tests/rescore_ref.py) is held to brute force (the packed forward
against every hypothesis scored on its own, the trie against a dictionary of prefixes), the cases of tests/rescore_cases.py are checked
for what they claim to cover, and the host side of the C ABI (exports, argument counts, refusals before any launch) is exercised."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import rescore_cases as RC
from tests import rescore_ref as RR

ROOT = Path(__file__).resolve().parents[1]
SMALL = [k for k in RC.CASES if k != "big"]
NEW = ("fk_nbest_trie", "fk_nbest_trie_mask", "fk_gpt_embed_pos", "fk_nbest_rescore")


@pytest.fixture(scope="module")
def built():
    from frankenstein_amd import build
    return build.build(verbose=False)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_packed_equals_flat(name):
    """every node sees exactly the causal context of its own flat sequence: |packed - flat| <= 1e-10 in float64, -inf in the same places"""
    case = RC.make(name)
    fin = np.isfinite(case["lm"])
    assert np.array_equal(fin, np.isfinite(case["packed"]))
    assert np.all(np.isneginf(case["lm"][~fin])) and np.all(np.isneginf(case["packed"][~fin]))
    err = np.abs(case["packed"][fin] - case["lm"][fin]).max()
    print(f"rescore {name}: |packed - flat| {err:.2e}, e32 {case['e32']:.2e}, smallest gap {case['gap']:.3f}, N {case['N']}")
    assert err <= 1e-10, (name, err)


@pytest.mark.parametrize("name", SMALL)
def test_trie_matches_a_dictionary(name):
    """the trie of the restatement against the set of distinct prefixes of the scored hypotheses, numbered by first appearance"""
    case = RC.make(name)
    ids, lengths, am = case["inp"].ids.numpy(), case["inp"].lengths.numpy(), case["inp"].am.numpy()
    for b, tr in enumerate(case["tries"]):
        lens = RR.clamp_lengths(lengths[b], case["T"])
        number = {(): 0}
        for h in range(case["n"]):
            seq = tuple(int(t) for t in ids[b, h, :lens[h]])
            if tr["leaf"][h] < 0:                                       # unscored: why?
                bad = (not np.isfinite(am[b, h])) or any(t < 0 or t >= case["V"] for t in seq)
                new = sum(1 for j in range(1, len(seq) + 1) if seq[:j] not in number)
                assert bad or len(number) + new > case["N"], (name, b, h)
                continue
            for j in range(1, len(seq) + 1):
                number.setdefault(seq[:j], len(number))
            assert tr["leaf"][h] == number[seq], (name, b, h)
        assert tr["n_nodes"] == len(number) <= case["N"]
        for p, i in number.items():
            assert tr["depth"][i] == len(p)
            if p:
                assert tr["tok"][i] == p[-1] and tr["parent"][i] == number[p[:-1]] < i
        dead = slice(tr["n_nodes"], None)
        assert np.all(tr["tok"][dead] == case["bos"]) and np.all(tr["depth"][dead] == 0) and np.all(tr["parent"][dead] == -1)


def test_cases_keep_their_purpose():
    """what the table of tests/rescore_cases.py says each case is for (make() itself asserts the margins of the ranking cases)"""
    e = RC.make("edits")
    lengths, am = e["inp"].lengths.numpy(), e["inp"].am.numpy()
    t0, t1, t2 = e["tries"]
    assert t0["leaf"][3] == t0["leaf"][1] > 0 and e["total"][0, 3] == e["total"][0, 1]            # the duplicate: an exact tie ...
    place = list(e["order"][0])
    assert place.index(3) == place.index(1) + 1                                                   # ... decided by the original index
    assert t0["leaf"][5] == 0 and lengths[0, 5] == 0 and np.isfinite(e["lm"][0, 5])                # the empty hypothesis is scored (end-of-text row)
    assert lengths[0, 6] == e["T"] and t0["leaf"][6] > 0                                          # a length at T
    assert list(t1["leaf"][[2, 4, 7]]) == [-1, -1, -1] and np.isneginf(am[1, 7]) and e["n_scored"][1] == e["n"] - 3
    assert list(e["order"][1][-3:]) == [2, 4, 7]                                                  # unscored: last, in original order
    assert lengths[2, 1] == e["T"] + 7 and lengths[2, 6] == -3 and t2["leaf"][6] == 0 and t2["depth"][t2["leaf"][1]] == e["T"]
    assert bool((e["inp"].ids == RC.GARBAGE).any()) and not e["inp"].ids.is_contiguous()           # garbage behind the lengths, strided
    assert RC.make("one")["n"] == 1 and RC.make("plain")["P"] == 0 and RC.make("plain")["eos"] is None
    assert 64 < RC.make("mid")["P"] + RC.make("mid")["N"] <= 128 < RC.make("wide")["P"] + RC.make("wide")["N"]
    assert RC.make("mid")["n"] == RC.make("wide")["n"] == 32
    o = RC.make("overflow")
    for b, mid in ((0, 2), (1, 3)):                                     # the long hypothesis does not fit, the later ones still do
        leaf = o["tries"][b]["leaf"]
        assert leaf[mid] == -1 and np.all(np.delete(leaf, mid) >= 0) and o["tries"][b]["n_nodes"] <= o["N"] == o["max_nodes"]
        assert np.isfinite(o["inp"].am.numpy()[b, mid])
    assert RC.make("big")["V"] == 50257 and RC.make("big")["eos"] == 50256
    for name in RC.RANKING:                                             # the order depends on the LM: with lm = 0 it is the identity
        case = RC.make(name)
        am = case["inp"].am.numpy()
        changed = False
        for b in range(case["B"]):
            scored = case["tries"][b]["leaf"] >= 0
            lens = RR.clamp_lengths(case["inp"].lengths.numpy()[b], case["T"])
            aw, lw, lb = case["weights"]
            _, order0, _ = RR.combine_rank(am[b], np.zeros(case["n"]), lens, scored, aw, lw, lb)
            changed |= not np.array_equal(order0, case["order"][b])
        assert changed, name


def test_exports_and_argument_counts(built):
    from frankenstein_amd import _lib
    header = (ROOT / "include" / "franken_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW:
        proto = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
        assert proto, f"{name} is not declared in include/franken_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.fk_version() == 302
    for macro, value in (("FK_NBEST_MAX_HYPS", _lib.NBEST_MAX_HYPS), ("FK_NBEST_MAX_T", _lib.NBEST_MAX_T), ("FK_NBEST_MAX_NODES", _lib.NBEST_MAX_NODES),
                         ("FK_NBEST_MAX_ROWS", _lib.NBEST_MAX_ROWS)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    from frankenstein_amd import kernels as K
    assert callable(K.head_ce_stats) and callable(K.nbest_trie) and callable(K.nbest_trie_mask) and callable(K.gpt_embed_pos) and callable(K.nbest_rescore)


def test_refusals_need_no_gpu(built):
    """every refusal returns -1 with its message before any launch"""
    from frankenstein_amd import _lib
    lib = _lib.lib()
    Q = 4096                                            # never dereferenced

    def trie(ids=Q, ldb=8 * 12, ldh=12, lengths=Q, B=2, n=8, T=12, V=307, bos=306, eos=-1, cap=40, P=0, tok=Q, leaf=Q, src=Q, tgt=Q):
        return lib.fk_nbest_trie(ids, ldb, ldh, lengths, None, B, n, T, V, bos, eos, cap, P, tok, Q, Q, leaf, Q, src, tgt, None)

    for kw, msg in [(dict(n=33), b"n = 33"), (dict(n=0), b"n = 0"), (dict(tok=None), b"null pointer"), (dict(ids=None), b"null pointer"),
                    (dict(leaf=None), b"null pointer"), (dict(cap=0), b"node_cap = 0"), (dict(cap=_lib.NBEST_MAX_NODES + 1), b"node_cap"),
                    (dict(T=0), b"T = 0"), (dict(T=_lib.NBEST_MAX_T + 1, ldh=2048, ldb=8 * 2048), b"T = 1025"), (dict(bos=307), b"bos = 307"),
                    (dict(eos=307), b"eos = 307"), (dict(ldh=11), b"ids strides"), (dict(src=None), b"come together"), (dict(B=0), b"B = 0")]:
        assert trie(**kw) == -1 and msg in lib.fk_last_error(), (kw, lib.fk_last_error())

    def mask(parent=Q, table=Q, B=2, P=5, N=40):
        return lib.fk_nbest_trie_mask(parent, Q, table, B, P, N, None)

    for kw, msg in [(dict(table=None), b"null pointer"), (dict(N=0), b"N = 0"), (dict(P=6, N=_lib.NBEST_MAX_ROWS - 5), b"envelope"), (dict(P=-1), b"P = -1")]:
        assert mask(**kw) == -1 and msg in lib.fk_last_error(), (kw, lib.fk_last_error())

    def embed(out=Q, prefix=Q, P=5, N=40, dtype=_lib.FK_F32, wpe_rows=64):
        return lib.fk_gpt_embed_pos(Q, Q, prefix, Q, Q, out, 2, P, N, 128, 307, wpe_rows, dtype, None)

    for kw, msg in [(dict(out=None), b"null pointer"), (dict(prefix=None), b"prefix is NULL"), (dict(dtype=7), b"dtype"), (dict(wpe_rows=5), b"wpe_rows = 5")]:
        assert embed(**kw) == -1 and msg in lib.fk_last_error(), (kw, lib.fk_last_error())

    def score(n=8, T=12, N=40, order=Q, row_m=Q, ldh=12):
        return lib.fk_nbest_rescore(row_m, Q, Q, Q, Q, Q, Q, Q, 8 * 12, ldh, Q, None, 2, n, T, N, 0, 1.0, 1.0, 0.0, -100, Q, Q, Q, Q, Q, Q, order, Q, None)

    for kw, msg in [(dict(n=33), b"n = 33"), (dict(order=None), b"null pointer (output)"), (dict(row_m=None), b"null pointer (input)"),
                    (dict(N=_lib.NBEST_MAX_ROWS + 1), b"N = 4097"), (dict(N=0), b"N = 0"), (dict(ldh=11), b"ids strides")]:
        assert score(**kw) == -1 and msg in lib.fk_last_error(), (kw, lib.fk_last_error())


def test_model_refusals_need_no_gpu():
    """GPT.score_nbest raises before any launch when the sequence does not fit block_size or the list is outside the envelope"""
    from frankenstein_amd.models.gpt2_model import GPT, GPTConfig
    m = GPT(GPTConfig(block_size=16, vocab_size=307, n_layer=1, n_head=2, n_embd=32))
    ids = torch.zeros((1, 2, 16), dtype=torch.int64)
    with pytest.raises(ValueError, match="block_size"):
        m.score_nbest(ids, torch.ones((1, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="block_size"):
        m.score_nbest(ids[:, :, :12], torch.ones((1, 2), dtype=torch.int64), prefix=torch.zeros(1, 4, 32))
    with pytest.raises(ValueError, match="envelope"):
        m.score_nbest(torch.zeros((1, 33, 4), dtype=torch.int64), torch.ones((1, 33), dtype=torch.int64))
    with pytest.raises(ValueError, match="vocabulary"):
        m.score_nbest(ids[:, :, :4], torch.ones((1, 2), dtype=torch.int64))           # the default start token 50256 against V = 307
