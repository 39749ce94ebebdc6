"""Every kernel fk_attn_fwd / fk_attn_bwd choose between (forward, dQ, dK/dV: generic, few-query, pre-scaled tile loops, generated
streams), against a float64 reference, on inputs where one lost key, one skipped tile of 64 keys, a ring slot read a tile late or a
mask edge off by one is an error of many times the bound (tests/attn_inputs.py: address-coded keys, queries aimed at the key at the
visible edge, at the hidden key behind it and at keys cycling through the key tiles; tests/test_attn_routes_cpu.py proves on the
reference alone that each of those defects moves some output by at least 2x the bound, on every case).

Before it launches, every test asks the host-side route query (kernels.attn_route, the function the launchers themselves ask) which
kernels its shape reaches and compares them with the routes its id names; the shapes live in tests/cases.py (ATTN_ROUTE_CASES,
ATTN_SPIKE_CASES) and tests/test_attn_routes_cpu.py pins the same table, and what it must cover, without a GPU.

Each case: q in its own buffer, k | v packed side by side, o, dq and dk | dv as views inside sentinel-filled buffers from the guard-band
allocator (the columns beside them must stay untouched); forward, then backward on the forward's o and lse; all five tensors compared
on every element:
    |got - ref| <= [2^-8 |ref| + 2^-8 mag, bf16 only] + 2e-5 + 2e-5 mag          lse: atol = rtol = 1e-4
with mag the float64 sum of the absolute terms of the last product (derivation: tests/attn_inputs.py).  delta = rowsum(dO * O) of the
reference uses the O the device returned.  Pre-scaled cases hand over Q' = scale log2(e) q (dyadic, exact in bf16) and the reference
uses Q' / (scale log2 e).  Prints "FRAC <tensor> <routes> <largest error / bound>".

No pair of kernels promises the same summation order (the generated streams and the tile loops split a row's keys differently), so
there is no bit-equality check between routes: the same data reaches the tile loops through a sliced mask and through ragged shapes,
and both sides are held to the bound.

FRAC maxima per route on the MI355X (every case passes; the CPU rounding model of tests/test_attn_routes_cpu.py peaks at 0.96 too):
  forward  o    FWD_GENERIC 0.77   FWD_FEWQ 0.47   FWD_PS 0.82   FWD_ASM 0.79          lse: at most 0.0014 on every route
  dQ       dq   DQ_GENERIC 0.73    DQ_FEWQ 0.67    DQ_PS 0.78    DQ_ASM 0.77
  dK/dV    dk   DKDV_GENERIC 0.89  DKDV_PS 0.91    DKDV_ASM 0.87 DKDVW_ASM 0.87
           dv   DKDV_GENERIC 0.90  DKDV_PS 0.96    DKDV_ASM 0.94 DKDVW_ASM 0.94"""
import pytest
import torch

from tests import attn_inputs as AI
from tests import cases

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
PAD = 8                         # elements on either side of a row: 16 bytes in bf16, 32 in fp32


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def guarded(B, N, H, D, dtype, parts=1):
    """`parts` [B, N, H, D] views side by side, PAD columns into the rows of a sentinel-filled [B, N, parts * H * D + 2 PAD] buffer"""
    buf = torch.zeros(B, N, parts * H * D + 2 * PAD, dtype=dtype, device="cuda")
    buf.fill_(SENTINEL)
    return buf, [buf[..., PAD + i * H * D:PAD + (i + 1) * H * D].unflatten(-1, (H, D)) for i in range(parts)]


def neighbours_untouched(buf):
    b = buf.float().cpu()
    return bool((b[..., :PAD] == SENTINEL).all()) and bool((b[..., -PAD:] == SENTINEL).all())


def check(name, routes, got, ref, mag, dtype):
    got = AI.heads(got.double().cpu())
    assert got.shape == ref.shape
    worst, at = AI.frac(got, ref, mag, dtype)
    print(f"FRAC {name} {'.'.join(routes)} {worst:.4f}")
    if not worst <= 1.0:
        idx = []
        for n in reversed(ref.shape):
            idx.insert(0, at % n)
            at //= n
        over = int(((got - ref).abs() > AI.bound(ref, mag, dtype)).sum())
        raise AssertionError(f"{name} on {routes}: error {worst:.3f} x its bound at [b, h, row, d] = {idx}: got {float(got[tuple(idx)])!r}, "
                             f"want {float(ref[tuple(idx)])!r}; {over} elements over")


def run_case(K, case):
    B, H, Nq, Nk, D, ps = case["B"], case["H"], case["Nq"], case["Nk"], case["D"], case["ps"]
    inp = AI.make_inputs(case)
    dtype, vis, scale = inp["dtype"], inp["vis"], inp["scale"]
    mask = AI.make_mask(K, case, inp["extras"], vis, "cuda")
    routes = K.attn_route_names(Nq, Nk, D, dtype, mask, q_prescaled=ps)
    assert routes == case["routes"], f"{case['id']} reaches {routes}"

    qbuf, (qd,) = guarded(B, Nq, H, D, dtype)
    kvbuf, (kd, vd) = guarded(B, Nk, H, D, dtype, parts=2)
    gbuf, (dod,) = guarded(B, Nq, H, D, dtype)
    for dst, src in ((qd, inp["q_dev"]), (kd, inp["k"]), (vd, inp["v"]), (dod, inp["do"])):
        dst.copy_(src.to(dtype))
        assert torch.equal(dst.double().cpu(), src)                            # the device holds the reference's operand values
    obuf, (o,) = guarded(B, Nq, H, D, dtype)
    _, lse = K.attn_fwd(qd, kd, vd, mask, scale=scale, out=o, q_prescaled=ps)

    q, k, v, do = (AI.heads(inp[n]) for n in ("q", "k", "v", "do"))
    oref, lref, mag_o, P = AI.forward(q, k, v, vis, scale)
    check("o", routes, o, oref, mag_o, dtype)
    lse_c = lse.double().cpu()
    dead = torch.isinf(lref)
    assert torch.equal(torch.isinf(lse_c) & (lse_c > 0), dead), "fully masked rows: lse = +inf, and only there"
    lerr = ((lse_c - lref)[~dead].abs() / (1e-4 + 1e-4 * lref[~dead].abs())).max()
    print(f"FRAC lse {'.'.join(routes)} {float(lerr):.4f}")
    assert float(lerr) <= 1.0
    assert neighbours_untouched(obuf)

    dqbuf, (dq,) = guarded(B, Nq, H, D, dtype)
    dkvbuf, (dk, dv) = guarded(B, Nk, H, D, dtype, parts=2)
    K.attn_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, mask, scale=scale, q_prescaled=ps)
    ref = AI.backward(q, k, v, do, P, AI.heads(o.double().cpu()), scale)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        check(name, routes, got, ref[name], ref["mag_" + name], dtype)
    assert neighbours_untouched(dqbuf) and neighbours_untouched(dkvbuf)
    assert neighbours_untouched(qbuf) and neighbours_untouched(kvbuf) and neighbours_untouched(gbuf)      # and the inputs are as they were
    assert torch.equal(qd.double().cpu(), inp["q_dev"]) and torch.equal(vd.double().cpu(), inp["v"])


@pytest.mark.parametrize("case", cases.ATTN_ROUTE_CASES, ids=lambda c: c["id"])
def test_attention_routes_against_float64(K, case):
    run_case(K, case)


@pytest.mark.parametrize("case", cases.ATTN_SPIKE_CASES, ids=lambda c: c["id"])
def test_attention_spikes_against_float64(K, case):
    """spike > 0: one key near the end scores 40 log2 units (plus its address digits) above 0 for one row per head, its other keys about
    40 below: the reference-0 loop runs for tiles on end, then its half-row sum leaves the safe range (exact loop; on the generated
    stream the whole workgroup redoes its rows).  spike < 0: every score of head 0 lies 2048 log2 units down, far below the window in
    which reference 0 is entered at all."""
    run_case(K, case)
