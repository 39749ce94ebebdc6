"""fk_augment_patchify (csrc/augment.hip) against the float64 restatement of tests/augment_ref.py on every case of
tests/augment_cases.py, in both compute dtypes.

Exact zeros: the set of exactly-zero output elements equals the restatement's (padding, out-of-range shift, dropped channels, spans, the
P <= p < ldp columns).  Non-zero elements: the device's fp32 chain (logf, sqrtf, sincospif, one fma, one add) is held to 4 x the largest
error of a numpy float32 evaluation of the same chain against the float64 rule on that case, plus half a bf16 ulp for a bf16 store; a case
without noise has the bound 0: x passes bit for bit.  tests/test_augment_cpu.py shows that every planted defect breaks this bound.
Prints "FRAC <case> <dtype> <error / bound>" (recorded in profiles/augment.md).

Bit for bit: an all-zero config equals fk_patchify; the fused tokens equal fk_patchify of the signal-mode output drawn with the same
words; the same words twice give the same bits.  Captured in a graph with augment_begin, two replays equal the restatement at steps
s + 1 and s + 2.  Every refusal leaves the output untouched.

Measured on the MI355X (profiles/augment.md): the fp32 error is at most 0.25 of its bound (6.9e-07 per unit sd at worst), in bf16 the
bound is the rounding of the store itself (1.000); cases without noise are exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import augment_ref as AR

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
_REF = {}


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import engine, kernels
    return engine, kernels


def ref_of(case):
    """x, float64 reference and bound of a case, computed once and shared by both dtypes"""
    if case.id not in _REF:
        x = case.x()
        _REF[case.id] = (x, *AR.bound(x, case.cfg, case.words, case.P, case.ldp))
    return _REF[case.id]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words_of(case):
    return torch.tensor(case.words, dtype=torch.int32, device="cuda")


def check(case, dtype, tok, ref, bnd, label):
    got = tok.double().cpu().numpy().reshape(ref.shape)
    assert np.array_equal(got == 0.0, ref == 0.0), (label, int(np.sum((got == 0.0) != (ref == 0.0))))
    assert not np.any(np.signbit(got) & (got == 0.0)), label                     # a masked element is +0
    lim = bnd + AR.half_ulp(ref, dtype) * (dtype == "bf16")
    err = np.abs(got - ref)
    worst = float(np.max(np.where(lim > 0, err / np.maximum(lim, 1e-300), np.where(err > 0, np.inf, 0.0))))
    sd = max(case.cfg.white_sd, case.cfg.offset_sd)
    print(f"FRAC {label} {dtype} {worst:.3f}  (max err {float(err.max()):.3e}, bound {bnd:.3e}, fp32 error per unit sd "
          f"{float(err.max()) / sd if sd and dtype == 'fp32' else float('nan'):.3e})")
    assert np.all(err <= lim), (label, worst, int(np.sum(~(err <= lim))))


ALL = [(c, dt) for c in AC.CASES for dt in c.dtypes]


@pytest.mark.parametrize("case,dtype", ALL, ids=lambda v: v.id if isinstance(v, AC.Case) else v)
def test_against_float64(mods, case, dtype):
    E, K = mods
    x, ref, bnd = ref_of(case)
    xg, words = cuda(x), words_of(case)
    tok = K.augment_patchify(xg, case.P, case.ldp, TDT[dtype], case.cfg, words)
    torch.cuda.synchronize()
    check(case, dtype, tok, ref, bnd, case.id)
    assert torch.equal(tok, K.augment_patchify(xg, case.P, case.ldp, TDT[dtype], case.cfg, words))          # the same words: the same bits
    # the fused tokens are fk_patchify of the signal-mode output drawn with the same words
    sig = K.augment_patchify(xg, 1, 1, torch.float32, case.cfg, words).view(case.B, case.T, case.C)
    assert torch.equal(tok, K.patchify(sig, case.P, case.ldp, TDT[dtype]))
    assert torch.equal(sig, E.augment_signal(xg, case.cfg, words))
    assert words.tolist() == list(case.words)                                                               # the launch does not advance the words


@pytest.mark.parametrize("shape", AC.SHAPES, ids=lambda s: "B%d_T%d_C%d_P%d_ld%d" % s)
def test_all_zero_config_is_patchify(mods, shape):
    E, K = mods
    B, T, C, P, ldp = shape
    x = torch.randn(B, T, C, device="cuda")
    x[0, 1] = 0.0
    x[-1, 0, 0] = -0.0
    words = torch.tensor([11, 5], dtype=torch.int32, device="cuda")
    for dt in (("fp32",) if (P, ldp) == (1, 1) else ("fp32", "bf16")):
        for cfg in (AR.Cfg(), AR.Cfg(keep_padding=False), AR.Cfg(n_time_masks=4, time_mask_len=0)):
            tok = K.augment_patchify(x, P, ldp, TDT[dt], cfg, words)
            plain = K.patchify(x, P, ldp, TDT[dt])
            assert torch.equal(tok.view(torch.int16 if dt == "bf16" else torch.int32), plain.view(torch.int16 if dt == "bf16" else torch.int32))


def test_steps_and_seeds_draw_different_noise(mods):
    E, K = mods
    case = AC.BY_ID["B2_T50_C256_P25_ld32-all"]
    x = cuda(case.x())
    outs = []
    for w in (case.words, (case.words[0], case.words[1] + 1), (case.words[0] + 1, case.words[1])):
        outs.append(K.augment_patchify(x, case.P, case.ldp, torch.float32, case.cfg, torch.tensor(w, dtype=torch.int32, device="cuda")))
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2]) and not torch.equal(outs[1], outs[2])


def test_captured_graph_draws_fresh_noise_on_every_replay(mods):
    E, K = mods
    case = AC.BY_ID["B3_T15_C40_P5_ld32-all"]
    x, _, _ = ref_of(case)
    xg = cuda(x)
    words = E.augment_words(xg.device)
    assert words.dtype == torch.int32 and words.shape == (2,) and E.augment_words(xg.device) is words
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up: the LDS attribute and the allocator
        E.augment_begin(xg.device)
        E.augment_tokens(xg, case.P, case.ldp, torch.bfloat16, case.cfg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    seed, s = words.tolist()
    assert seed == E.augment_seed(torch.initial_seed(), 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                      # one chain: the increment, then the launch
        E.augment_begin(xg.device)
        tok = E.augment_tokens(xg, case.P, case.ldp, torch.bfloat16, case.cfg)
    seen = []
    for k in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        assert words.tolist() == [seed, s + k]
        ref, bnd = AR.bound(x, case.cfg, (seed, s + k), case.P, case.ldp)
        check(case, "bf16", tok, ref, bnd, f"graph replay {k}")
        seen.append(tok.clone())
    assert not torch.equal(seen[0], seen[1])


def test_refusals_write_nothing(mods):
    E, K = mods
    from frankenstein_amd import _lib
    lib = _lib.lib()
    B, T, C, P, ldp = 2, 8, 8, 4, 4
    x = torch.randn(B, T, C, device="cuda")
    words = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    tok = K.torch.empty((B * (T // P) * C, ldp), dtype=torch.float32, device="cuda")      # guard-banded under the suite's poison fixture
    tok.fill_(float("nan"))
    before = tok.view(torch.int32).clone()
    good = dict(white_sd=0.5, offset_sd=0.1, chan_drop_p=0.1, time_shift=1, n_time_masks=2, time_mask_len=3, keep_padding=1)

    def go(T_=T, P_=P, ldp_=ldp, C_=C, dtype=_lib.FK_F32, xp=x.data_ptr(), wp=words.data_ptr(), **knobs):
        k = dict(good)
        k.update(knobs)
        cfg = _lib.AugmentCfg(k["white_sd"], k["offset_sd"], k["chan_drop_p"], k["time_shift"], k["n_time_masks"], k["time_mask_len"], k["keep_padding"], 0)
        return lib.fk_augment_patchify(xp, tok.data_ptr(), B, T_, C_, P_, ldp_, ctypes.byref(cfg), wp, dtype, None)

    refused = [go(xp=None), go(wp=None), go(P_=3), go(ldp_=3), go(T_=4096, P_=4096, ldp_=4096), go(white_sd=-1.0), go(white_sd=float("inf")),
               go(offset_sd=float("nan")), go(chan_drop_p=1.0), go(chan_drop_p=-0.5), go(n_time_masks=9), go(n_time_masks=-1),
               go(time_mask_len=T + 1), go(time_mask_len=-1), go(time_shift=T), go(time_shift=-1), go(dtype=2)]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert torch.equal(tok.view(torch.int32), before)
    assert go() == 0                                                 # and the same call with legal knobs runs
    torch.cuda.synchronize()
    assert not torch.isnan(tok).any()
    with pytest.raises(_lib.FrankenHipError, match="chan_drop_p"):
        K.augment_patchify(x, P, ldp, torch.float32, AR.Cfg(chan_drop_p=1.0), words)
