"""fk_day_adapter_fwd / fk_day_adapter_bwd (csrc/dayadapt.hip) and the autograd Functions on them (engine.DayPatchify, PatchEmbedTok,
MaskedPatchEmbedTok) against the float64 restatement of tests/day_adapter_ref.py, on every case of tests/day_adapter_cases.py, in both
compute dtypes.

Kernels.  Bound per tensor: 4 x max |torch's own fp32 CPU composition - float64| of the same tensor (the project's usual yardstick);
the forward gets, per element, half an ulp of the output dtype at the reference value on top, for its one rounding.  The gradient
buffers are filled with NaN beforehand: a day absent from the batch must come back as exact zeros.  Padded columns are exactly zero,
out-of-range samples equal fk_patchify's rows, two runs give the same bits.  Prints "FRAC <case> <dtype> <tensor> <error / bound>".
tests/test_day_adapter_cpu.py shows that every planted defect of the restatement breaks these bounds.

Functions.  The gradients of DayPatchify -> PatchEmbedTok / MaskedPatchEmbedTok under a random upstream gradient.  The operands of every
product (upstream gradient, tokens, weight shadow) are values of the compute dtype and the sums are fp32, so the float64 reference is
taken on those operand values and the bound is the forward error bound of an fp32 sum of n terms in any order, n * 2^-24 * sum |a| |b|
(Higham, Accuracy and Stability of Numerical Algorithms, (3.5) with gamma_n ~ n u), chained through d_tok for d_delta and d_bias.

Measured on the MI355X, largest error / bound over the cases (profiles/day_adapter.md): tok 0.61 (fp32) and 1.00 (bf16: the bound is
the rounding of the store itself), d_delta 0.47, d_bias 0.62; Functions at most 0.018 in either mode."""
import numpy as np
import pytest
import torch

from tests import day_adapter_cases as DC
from tests import day_adapter_ref as DR

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
_REF = {}


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import frankenstein_amd as fa
    from frankenstein_amd import engine, kernels
    yield engine, kernels
    fa.set_compute_dtype("bf16")


def ref_of(case):
    """inputs, float64 reference and yardsticks of a case, computed once"""
    if case.id not in _REF:
        inp = case.inputs()
        ref, bnd = DR.bounds(*inp, case.P, case.ldp)
        _REF[case.id] = (inp, ref, bnd)
    return _REF[case.id]


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_kernels(K, case, dtype, inp):
    x, day, delta, bias, d_tok = (cuda(a) for a in inp)
    tok = K.day_adapter_fwd(x, day, delta, bias, case.P, case.ldp, TDT[dtype])
    out = (torch.full((case.n_days, case.C, case.C), float("nan"), device="cuda"), torch.full((case.n_days, case.C), float("nan"), device="cuda"))
    K.day_adapter_bwd(x, day, d_tok.view(-1, case.ldp), case.P, delta.shape, out=out)
    return tok.view(case.B, -1, case.ldp), out[0], out[1]


ALL = [(c, dt) for c in DC.CASES + DC.ROUTE_CASES for dt in c.dtypes]


@pytest.mark.parametrize("case,dtype", ALL, ids=lambda v: v.id if isinstance(v, DC.Case) else v)
def test_kernels_against_float64(mods, case, dtype):
    E, K = mods
    inp, ref, bnd = ref_of(case)
    x, day, delta, bias, d_tok = inp
    tok, d_delta, d_bias = run_kernels(K, case, dtype, inp)
    torch.cuda.synchronize()
    got = (tok.double().cpu().numpy(), d_delta.double().cpu().numpy(), d_bias.double().cpu().numpy())
    lims = (bnd[0] + DR.half_ulp(ref[0], dtype), bnd[1], bnd[2])
    fails = []
    for name, g, r, lim in zip(("tok", "d_delta", "d_bias"), got, ref, lims):
        err = np.abs(g - r)
        bad = ~(err <= lim)                                       # NaN counts as bad
        worst = float(np.max(np.where(np.asarray(lim) > 0, err / np.maximum(lim, 1e-300), np.where(err > 0, np.inf, 0.0))))
        print(f"FRAC {case.id} {dtype} {name} {worst:.3f}  (max err {float(np.nanmax(err)):.3e}, yardstick {float(np.max(lim)):.3e})")
        if bad.any():
            fails.append((name, int(bad.sum()), worst))
    assert not fails, fails
    # padded columns are exactly zero
    assert float(tok[:, :, case.P:].abs().max() if case.ldp > case.P else 0.0) == 0.0
    # a sample without a valid day equals fk_patchify's rows (bit for bit), and absent days have exact-zero gradients
    plain = K.patchify(cuda(x), case.P, case.ldp, TDT[dtype]).view(case.B, -1, case.ldp)
    _, ok = DR.valid_days(day, case.B, case.n_days)
    for b in range(case.B):
        if not ok[b]:
            assert torch.equal(tok[b], plain[b]), b
    present = set(np.asarray(day)[ok].tolist()) if day is not None else set()
    for d in range(case.n_days):
        if d not in present:
            assert float(d_delta[d].abs().max()) == 0.0 and float(d_bias[d].abs().max()) == 0.0, d
    # determinism: the same bits on a second run
    tok2, dd2, db2 = run_kernels(K, case, dtype, inp)
    assert torch.equal(tok, tok2) and torch.equal(d_delta, dd2) and torch.equal(d_bias, db2)


@pytest.mark.parametrize("case,dtype", [(c, dt) for c in DC.CASES + DC.ROUTE_CASES if c.pattern in ("different", "outrange", "mixed") for dt in c.dtypes],
                         ids=lambda v: v.id if isinstance(v, DC.Case) else v)
def test_zero_adapter_is_patchify(mods, case, dtype):
    E, K = mods
    x, day, delta, bias, _ = case.inputs()
    xg = cuda(x)
    tok = K.day_adapter_fwd(xg, cuda(day), torch.zeros_like(cuda(delta)), torch.zeros_like(cuda(bias)), case.P, case.ldp, TDT[dtype])
    assert torch.equal(tok, K.patchify(xg, case.P, case.ldp, TDT[dtype]))
    tok = K.day_adapter_fwd(xg, None, cuda(delta), cuda(bias), case.P, case.ldp, TDT[dtype])          # day = NULL: all pass through
    assert torch.equal(tok, K.patchify(xg, case.P, case.ldp, TDT[dtype]))


def test_graph_capture_follows_the_day_tensor(mods):
    E, K = mods
    case = DC.BY_ID["B4_T32_C16_P4_ld32_D3-different"]
    x, day, delta, bias, d_tok = (cuda(a) for a in case.inputs())
    d_tok = d_tok.view(-1, case.ldp)
    day_static = day.clone()
    out = (torch.empty((case.n_days, case.C, case.C), device="cuda"), torch.empty((case.n_days, case.C), device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up: the LDS attribute and the allocator
        K.day_adapter_fwd(x, day_static, delta, bias, case.P, case.ldp, torch.bfloat16)
        K.day_adapter_bwd(x, day_static, d_tok, case.P, delta.shape, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tok = K.day_adapter_fwd(x, day_static, delta, bias, case.P, case.ldp, torch.bfloat16)
        K.day_adapter_bwd(x, day_static, d_tok, case.P, delta.shape, out=out)
    seen = []
    for days in ([0, 1, 2, 0], [2, 2, -1, 1], [3, 0, 0, 0]):
        day_static.copy_(torch.tensor(days, device="cuda"))
        g.replay()
        torch.cuda.synchronize()
        d = torch.tensor(days, device="cuda")
        eager_tok = K.day_adapter_fwd(x, d, delta, bias, case.P, case.ldp, torch.bfloat16)
        eager = K.day_adapter_bwd(x, d, d_tok, case.P, delta.shape)
        assert torch.equal(tok, eager_tok) and torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]), days
        seen.append(tok.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


U = 2.0 ** -24


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("masked", [False, True], ids=["PatchEmbedTok", "MaskedPatchEmbedTok"])
def test_functions_against_float64(mods, dtype, masked):
    E, K = mods
    import frankenstein_amd as fa
    fa.set_compute_dtype(dtype)
    B, T, C, P, n_days, d = 4, 32, 16, 4, 3, 32
    kp, nT = 32, T // P
    N = nT * C
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    day = np.array([2, 0, -1, 2], dtype=np.int64)
    delta = (rng.standard_normal((n_days, C, C)) / np.sqrt(C)).astype(np.float32)
    bias = (rng.standard_normal((n_days, C)) + np.arange(n_days)[:, None]).astype(np.float32)
    P_ = lambda a: torch.nn.Parameter(cuda(a.astype(np.float32)))
    p_delta, p_bias = P_(delta), P_(bias)
    emb_w, emb_b, space = P_(rng.standard_normal((d, P)) * 0.5), P_(rng.standard_normal(d)), P_(rng.standard_normal((1, C, d)))
    tok, carrier = E.DayPatchify.apply(cuda(x), cuda(day), p_delta, p_bias, P, kp, False, True)
    assert carrier.shape == tok.shape and carrier.dtype == torch.float32 and carrier.stride() == (0, 0, 0)
    assert tok.shape == (B, N, kp) and tok.dtype == TDT[dtype]
    if masked:
        n = N // 4
        unm = torch.stack([torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(b))[:n])[0] for b in range(B)]).cuda()
        h = E.MaskedPatchEmbedTok.apply(tok, emb_w, emb_b, space, unm, P, carrier)
        rows = (torch.arange(B)[:, None] * N + unm.cpu()).reshape(-1).numpy()
    else:
        h = E.PatchEmbedTok.apply(tok, emb_w, emb_b, space, P, carrier)
        rows = np.arange(B * N)
    G = torch.randn(h.shape, generator=torch.Generator().manual_seed(3)).to(TDT[dtype]).cuda()
    h.backward(G)
    torch.cuda.synchronize()
    # float64 reference on the operand values the kernels see
    rnd = lambda a: DR.round_to(a, dtype)
    g2 = G.double().cpu().numpy().reshape(-1, d)
    tok2 = tok.detach().double().cpu().numpy().reshape(B * N, kp)[rows]
    Wc = rnd(emb_w.detach().double().cpu().numpy())
    R = g2.shape[0]
    ch = rows % C
    ref = {"emb_w": g2.T @ tok2[:, :P], "emb_b": g2.sum(0), "space": np.stack([g2[ch == c].sum(0) for c in range(C)])[None]}
    lim = {"emb_w": R * U * (np.abs(g2).T @ np.abs(tok2[:, :P])), "emb_b": R * U * np.abs(g2).sum(0),
           "space": R * U * np.stack([np.abs(g2[ch == c]).sum(0) for c in range(C)])[None]}
    d_tok = np.zeros((B * N, kp))
    e_tok = np.zeros((B * N, kp))
    d_tok[rows, :P] = g2 @ Wc
    e_tok[rows, :P] = d * U * (np.abs(g2) @ np.abs(Wc))
    ref["delta"], ref["bias"] = DR.backward(x, day, d_tok.reshape(B, N, kp), P, n_days)
    ax, adt = np.abs(x.astype(np.float64)), np.abs(d_tok).reshape(B, N, kp)
    n_sum = B * T
    m_delta, m_bias = DR.backward(ax, day, adt, P, n_days)                                   # sum |x| |dy|, sum |dy|
    p_delta_e, p_bias_e = DR.backward(ax, day, e_tok.reshape(B, N, kp), P, n_days)            # the error of d_tok carried through
    lim["delta"], lim["bias"] = n_sum * U * m_delta + p_delta_e, n_sum * U * m_bias + p_bias_e
    got = {"emb_w": emb_w.grad, "emb_b": emb_b.grad, "space": space.grad, "delta": p_delta.grad, "bias": p_bias.grad}
    fails = []
    for name in ref:
        g = got[name].double().cpu().numpy()
        assert g.shape == ref[name].shape, name
        err = np.abs(g - ref[name])
        worst = float(np.max(np.where(lim[name] > 0, err / np.maximum(lim[name], 1e-300), np.where(err > 0, np.inf, 0.0))))
        print(f"FRAC functions {'masked' if masked else 'plain'} {dtype} {name} {worst:.3f}")
        if not np.all(err <= lim[name]):
            fails.append((name, worst))
    assert not fails, fails
    assert float(p_delta.grad[1].abs().max()) == 0.0 and float(p_bias.grad[1].abs().max()) == 0.0        # day 1 is absent
    assert float(np.abs(ref["delta"][2]).max()) > 1.0                                                    # and the present ones are not small


def test_functions_without_a_carrier(mods):
    """DayPatchify.apply(x, day, delta, bias, P, ldp) -> tok alone: the gradient reaches the adapter through tok (fp32 mode: unrounded)"""
    E, K = mods
    import frankenstein_amd as fa
    fa.set_compute_dtype("fp32")
    case = DC.BY_ID["B4_T32_C16_P4_ld32_D3-different"]
    inp, ref, bnd = ref_of(case)
    x, day, delta, bias, d_tok = inp
    pd, pb = torch.nn.Parameter(cuda(delta)), torch.nn.Parameter(cuda(bias))
    tok = E.DayPatchify.apply(cuda(x), cuda(day), pd, pb, case.P, case.ldp)
    assert torch.equal(tok.view(-1, case.ldp), K.day_adapter_fwd(cuda(x), cuda(day), cuda(delta), cuda(bias), case.P, case.ldp, torch.float32))
    tok.backward(cuda(d_tok))
    assert np.all(np.abs(pd.grad.double().cpu().numpy() - ref[1]) <= bnd[1]) and np.all(np.abs(pb.grad.double().cpu().numpy() - ref[2]) <= bnd[2])


def test_day_adapter_module(mods):
    """brainformer.DayAdapter: the P = 1 mode returns the adapted [B, T, C] signal in fp32 and trains delta and bias"""
    E, K = mods
    from frankenstein_amd.models.brainformer import DayAdapter
    case = DC.BY_ID["B2_T33_C256_P1_ld1_D2-different"]
    inp, ref, bnd = ref_of(case)
    x, day, delta, bias, d_tok = inp
    ad = DayAdapter(case.n_days, case.C).cuda()
    assert torch.equal(ad(cuda(x), cuda(day)), cuda(x)) and torch.equal(ad(cuda(x), None), cuda(x))      # fresh: the identity
    with torch.no_grad():
        ad.delta.copy_(cuda(delta))
        ad.bias.copy_(cuda(bias))
    y = ad(cuda(x), torch.from_numpy(day).int())                    # int32 on the host is one of the accepted forms
    assert y.shape == x.shape and y.dtype == torch.float32
    y.backward(cuda(d_tok).view(x.shape))
    got = (y.detach().double().cpu().numpy().reshape(ref[0].shape), ad.delta.grad.double().cpu().numpy(), ad.bias.grad.double().cpu().numpy())
    for g, r, lim in zip(got, ref, (bnd[0] + DR.half_ulp(ref[0], "fp32"), bnd[1], bnd[2])):
        assert np.all(np.abs(g - r) <= lim)
    assert torch.equal(ad(cuda(x), 1), ad(cuda(x), torch.tensor([1, 1])))                                 # a Python int is broadcast
