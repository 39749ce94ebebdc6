"""CPU-side checks of nucleus (top-p) sampling: fk_sample_topp is exported and bound and refuses what lies outside its envelope on the host
(FK_EINVAL before any launch; the pointers are small fake addresses, so every call has exactly one thing wrong with it), the host-tensor
form of GPT._sample draws from exactly the set the rule keeps, and GPT.generate / Franky.generate refuse a top_p outside (0, 1].

`nucleus_ref` (tests/sample_ref.py) is the float64 numpy restatement of the rule in include/franken_hip.h (fk_sample_topp);
tests/test_nucleus_gpu.py holds the kernel to the same function.  It also returns the MARGIN of a case,
min_i |mass_gt(i) / total - top_p| over the tokens the top-k crop keeps:
the header lets a token closer than 1e-4 to the boundary fall on either side, so every case first asserts a margin >= 0.02 (a condition on
its inputs; the crafted rows below give 0.03 .. 0.08)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.sample_ref import MIN_MARGIN, nucleus_ref  # noqa: F401  (moved there; tests/test_nucleus_gpu.py imports both from here)

EINVAL = -1
P = 4096          # a fake, 16-byte aligned "device pointer": never dereferenced by a refused call

# The crafted row: six head tokens with these probabilities, the remaining .11 spread over all other tokens as one identical float.
# mass_gt / total of the heads and the tail: 0, .30, .50, .65, .75, .83, .89
HEADS = (0.30, 0.20, 0.15, 0.10, 0.08, 0.06)
POS_1000 = (611, 7, 999, 130, 0, 448)            # head j of the V = 1000 rows sits at POS_1000[j]: scattered, both ends included


def crafted_row(V, positions, temperature, shift=0.0):
    """fp32 [V]: logits = temperature * (log p + shift), so that logits / temperature is log p (+ shift) again"""
    p = np.full(V, (1.0 - sum(HEADS)) / (V - len(HEADS)), np.float64)
    p[list(positions)] = HEADS
    return (temperature * (np.log(p) + shift)).astype(np.float32)


# (top_p, top_k) -> how many of the heads stay, and whether the tail does
CASES = {(0.25, None): (1, False), (0.45, None): (2, False), (0.70, None): (4, False), (0.92, None): (6, True), (0.70, 5): (3, False),
         (0.50, 3): (2, False)}


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("case", sorted(CASES, key=str), ids=lambda c: f"p{c[0]}-k{c[1]}")
def test_the_restatement_on_the_crafted_row(case, T):
    """the kept sets the cases are named for, and the margins the GPU tests rely on"""
    top_p, top_k = case
    heads, tail = CASES[case]
    kept, margin, probs = nucleus_ref(crafted_row(1000, POS_1000, T), T, top_k, top_p)
    assert margin >= MIN_MARGIN, margin
    assert [bool(kept[i]) for i in POS_1000] == [j < heads for j in range(6)]
    assert int(kept.sum()) == heads + (994 if tail else 0)
    assert abs(probs.sum() - 1.0) < 1e-12 and probs[POS_1000[0]] == probs.max()


@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_export_exists(lib):
    from frankenstein_amd import _lib
    h = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(h, "fk_sample_topp") and "fk_sample_topp" in _lib.SIGNATURES
    eos_args = _lib.SIGNATURES["fk_sample_topk_eos"][1]
    assert _lib.SIGNATURES["fk_sample_topp"][1] == eos_args[:6] + [ctypes.c_float] + eos_args[6:]      # top_p behind top_k, nothing else moves
    from frankenstein_amd import kernels as K
    assert callable(K.sample_topp)


def topp(lib, logits=P, ld=211, B=5, V=211, temperature=1.0, top_k=10, top_p=0.9, seed=P, step=P, pos_inc=P, cur=P, out=P, out_ld=8, out_cols=8,
         ticket=P, eos=7, done=P, len_=P, live_acc=P, live=P):
    return lib.fk_sample_topp(logits, ld, B, V, temperature, top_k, top_p, seed, step, pos_inc, cur, out, out_ld, out_cols, ticket, eos, done, len_,
                              live_acc, live, None)


PLAIN = dict(done=None, len_=None, live_acc=None, live=None)


@pytest.mark.parametrize("mode", [{}, PLAIN], ids=["eos", "plain"])
def test_sample_topp_refuses_bad_arguments(lib, mode):
    for p in (0.0, -0.5, 1.5, math.nan, math.inf):
        assert topp(lib, top_p=p, **mode) == EINVAL and b"fk_sample_topp: need 0 < top_p <= 1" in lib.fk_last_error(), p
    for name in ("logits", "seed", "step", "cur", "ticket"):
        assert topp(lib, **{**mode, name: None}) == EINVAL and b"fk_sample_topp: null pointer" in lib.fk_last_error(), name
    assert topp(lib, out_cols=0, **mode) == EINVAL and b"fk_sample_topp" in lib.fk_last_error() and b"out_cols" in lib.fk_last_error()
    assert topp(lib, out_cols=9, **mode) == EINVAL and b"fk_sample_topp" in lib.fk_last_error()      # wider than its row stride
    assert topp(lib, B=0, **mode) == EINVAL and b"fk_sample_topp" in lib.fk_last_error()
    assert topp(lib, ld=210, **mode) == EINVAL and b"fk_sample_topp" in lib.fk_last_error()
    assert topp(lib, V=1 << 31, ld=1 << 31, **mode) == EINVAL
    for t in (0.0, -1.0):
        assert topp(lib, temperature=t, **mode) == EINVAL and b"temperature" in lib.fk_last_error(), t


def test_sample_topp_refuses_a_partial_end_of_text_state(lib):
    names = ("done", "len_", "live_acc", "live")
    for bits in range(1, 15):                                                                          # every mixture: neither all four nor none
        missing = {n: None for i, n in enumerate(names) if bits >> i & 1}
        assert topp(lib, **missing) == EINVAL, missing
        assert b"fk_sample_topp" in lib.fk_last_error() and b"all four or none" in lib.fk_last_error(), missing
    assert topp(lib, eos=1 << 31) == EINVAL and b"fk_sample_topp: need eos < 2^31" in lib.fk_last_error()
    assert topp(lib, eos=1 << 31, top_p=0.0, **PLAIN) == EINVAL and b"top_p" in lib.fk_last_error()    # the plain mode does not read eos


# =============================================================================================== GPT._sample on host tensors
N_DRAWS = 4000


def host_draws(T, top_k, top_p, seed=11, **kw):
    from frankenstein_amd.models.gpt2_model import GPT
    row = torch.from_numpy(crafted_row(1000, POS_1000, T))
    torch.manual_seed(seed)
    if top_p == "absent":
        return GPT._sample(row.expand(N_DRAWS, -1), T, top_k, **kw).view(-1)
    return GPT._sample(row.expand(N_DRAWS, -1), T, top_k, top_p=top_p, **kw).view(-1)


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("case", sorted(CASES, key=str), ids=lambda c: f"p{c[0]}-k{c[1]}")
def test_host_sample_draws_from_the_kept_set_and_from_all_of_it(case, T):
    """4000 seeded draws: .25 only the argmax, .45 the first two heads, .70 the first four, .70 behind top_k = 5 the first three (top_p applies
    to the distribution renormalised after the crop), .92 reaches the tail (994 equal logits: they all stay)"""
    top_p, top_k = case
    heads, tail = CASES[case]
    kept, margin, probs = nucleus_ref(crafted_row(1000, POS_1000, T), T, top_k, top_p)
    assert margin >= MIN_MARGIN
    tok = host_draws(T, top_k, top_p)
    cnt = np.bincount(tok.numpy(), minlength=1000)
    assert int(cnt[~kept].sum()) == 0
    assert all(cnt[POS_1000[j]] > 0 for j in range(heads))
    n_tail = N_DRAWS - int(cnt[list(POS_1000)].sum())
    if tail:
        assert abs(n_tail / N_DRAWS - 0.11) <= 5 * math.sqrt(0.11 * 0.89 / N_DRAWS), n_tail
    else:
        assert n_tail == 0
        tv = 0.5 * float(np.abs(cnt / N_DRAWS - probs).sum())
        assert tv < 2.5 * math.sqrt(heads / (2 * math.pi * N_DRAWS)), tv


@pytest.mark.parametrize("top_k", [None, 5])
def test_host_sample_without_a_nucleus_is_unchanged(top_k):
    want = host_draws(0.7, top_k, "absent")
    assert torch.equal(host_draws(0.7, top_k, None), want) and torch.equal(host_draws(0.7, top_k, 1.0), want)
    assert not torch.equal(host_draws(0.7, top_k, 0.45), want)


def test_host_sample_keeps_ties_at_the_boundary_together():
    """two equal logits straddle the boundary (.40 | .25 .25 | .10): at top_p = .5 the first of the pair has .40 above it and stays, so both do"""
    from frankenstein_amd.models.gpt2_model import GPT
    row = torch.log(torch.tensor([[0.10, 0.25, 0.40, 0.25]]))
    torch.manual_seed(3)
    tok = GPT._sample(row.expand(2000, -1), 1.0, None, top_p=0.5).view(-1)
    assert sorted(set(tok.tolist())) == [1, 2, 3]
    kept, _, _ = nucleus_ref(row[0].numpy(), 1.0, None, 0.5)
    assert kept.tolist() == [False, True, True, True]


@pytest.mark.parametrize("bad", [0, 0.0, -0.1, 1.5, math.nan])
def test_generate_refuses_a_top_p_outside_its_range(bad):
    from frankenstein_amd.models.gpt2_model import GPT, GPTConfig
    from frankenstein_amd.models.notebook_models import Franky
    g = GPT(GPTConfig(block_size=16, vocab_size=32, n_layer=1, n_head=2, n_embd=16, dropout=0.0, bias=True))
    ids = torch.zeros((1, 1), dtype=torch.long)
    with pytest.raises(ValueError, match="top_p"):
        g.generate(ids, 2, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        g.generate(ids, 2, top_p=bad, eos_token_id=3)
    with pytest.raises(ValueError, match="top_p"):
        GPT._sample(torch.zeros(1, 32), 1.0, None, top_p=bad)
    fr = Franky(torch.nn.Identity(), g)
    for stop in (False, True):
        with pytest.raises(ValueError, match="top_p"):
            fr.generate(np.zeros((4, 2), np.float32), 2, top_p=bad, stop=stop)
