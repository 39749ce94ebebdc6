"""attn_bwd with a rope_table: the inverse rotation fused into the dQ and dK stores, on every kernel that has such a store (generic,
pre-scaled tile loops, the generated dQ stream and the narrow and wide dK/dV streams: store_rows_T_rope in csrc/attention.hip), called
the way engine.AttnBranch.run_backward calls it and held to a float64 reference on every element.

Each case (tests/cases.py ATTN_ROPE_CASES; tests/test_attn_rope_cpu.py pins their routes and what they cover): q | k | v are the three
views of one sentinel-filled [B, N, 3 H D + 2 PAD] buffer and dq | dk | dv those of a second one, o and dO live in guarded buffers of
their own; the table is shared [Tc, D/2, 2], per-sample [B, Tc, D/2, 2], or the [:, :Tc] slice of a taller per-sample buffer (batch
stride > Tc D), with Tc = rope_off + N.  The routes are asserted before the launch; attn_fwd, then attn_bwd(rope_table=, rope_off=,
q_prescaled=) on the forward's o and lse.  o, lse, dq, dk and dv are compared on every element with the dense float64 softmax of
tests/attn_inputs.py, its dq and dk un-rotated in float64 at the table's fp32 values:
    |got - ref'| <= [2^-8 |ref'| + 2^-8 mag', bf16 only] + 2e-5 + 2e-5 mag'          lse: atol = rtol = 1e-4
with mag0' = |c| mag0 + |s| mag1, mag1' = |s| mag0 + |c| mag1 (the rotation is linear with coefficients of at most 1, so the dS and fp32
terms of the bound carry over with mag'; the kernels rotate their fp32 accumulators and round once at the store: 2^-8 |ref'|).  The
sentinels beside every view must be intact and q, k, v, dO and the table unchanged.

The inputs are those of the route tests; the angles (attn_inputs.rope_table) are (pi / 2) m + pi / 8 + (pi / 4) u, unrelated between
rows, pairs and samples, so no rotation, the forward rotation, a table row one off, a forgotten rope_off or batch stride, a neighbouring
pair's angle or exchanged halves in the half-wave store are each at least 2x the bound in nearly every row (tests/test_attn_rope_cpu.py
proves that on the reference alone).  Prints "FRAC <tensor> <routes> <largest error / bound>".

FRAC maxima per route on the MI355X (every case passes; the CPU rounding model peaks at 0.91):
  forward  o    FWD_GENERIC 0.80   FWD_PS 0.82    FWD_ASM 0.79                         lse: at most 0.0014 on every route
  dQ       dq   DQ_GENERIC 0.73    DQ_PS 0.82     DQ_ASM 0.72
  dK/dV    dk   DKDV_GENERIC 0.78  DKDV_PS 0.89   DKDV_ASM 0.85  DKDVW_ASM 0.92
           dv   DKDV_GENERIC 0.89  DKDV_PS 0.89   DKDV_ASM 0.90  DKDVW_ASM 0.89"""
import pytest
import torch

from tests import attn_inputs as AI
from tests import cases
from tests.test_attn_routes_gpu import PAD, check, guarded, neighbours_untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def device_table(case):
    """-> (the table attn_bwd is handed, the float32 CPU table [Bt, Tc, D/2, 2] the reference uses)"""
    tall, Tc = AI.case_table(case)
    dev = tall.cuda()
    if case["table"] == "shared":
        tab = dev[0, :Tc].contiguous()
        assert tab.dim() == 3
    elif case["table"] == "sample":
        tab = dev[:, :Tc].contiguous()
        assert tab.stride(0) == Tc * case["D"]
    else:
        tab = dev[:, :Tc]
        assert tab.stride(0) == (Tc + AI.ROPE_SLACK) * case["D"] > Tc * case["D"]
    assert tab.stride()[-3:] == (case["D"], 2, 1) and tab.data_ptr() % 16 == 0
    return tab, tall[:, :Tc]


@pytest.mark.parametrize("case", cases.ATTN_ROPE_CASES, ids=lambda c: c["id"])
def test_fused_inverse_rope_against_float64(K, case):
    B, H, N, D, ps, off = case["B"], case["H"], case["Nq"], case["D"], case["ps"], case["rope_off"]
    inp = AI.make_inputs(case)
    dtype, vis, scale = inp["dtype"], inp["vis"], inp["scale"]
    mask = AI.make_mask(K, case, inp["extras"], vis, "cuda")
    routes = K.attn_route_names(N, N, D, dtype, mask, q_prescaled=ps, rope=True)
    assert routes == case["routes"], f"{case['id']} reaches {routes}"
    assert routes[0] == K.attn_route_names(N, N, D, dtype, mask, q_prescaled=ps)[0]              # the forward never sees the table

    qkvbuf, (qd, kd, vd) = guarded(B, N, H, D, dtype, parts=3)
    assert qkvbuf.shape == (B, N, 3 * H * D + 2 * PAD)
    gbuf, (dod,) = guarded(B, N, H, D, dtype)
    for dst, src in ((qd, inp["q_dev"]), (kd, inp["k"]), (vd, inp["v"]), (dod, inp["do"])):
        dst.copy_(src.to(dtype))
        assert torch.equal(dst.double().cpu(), src)                            # the device holds the reference's operand values
    obuf, (o,) = guarded(B, N, H, D, dtype)
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

    tab, tab_cpu = device_table(case)
    before = tab.clone()
    dbuf, (dq, dk, dv) = guarded(B, N, H, D, dtype, parts=3)
    K.attn_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, mask, scale=scale, rope_table=tab, rope_off=off, q_prescaled=ps)
    ref = AI.unrotate_grads(AI.backward(q, k, v, do, P, AI.heads(o.double().cpu()), scale), tab_cpu, off)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        check(name, routes, got, ref[name], ref["mag_" + name], dtype)
    assert neighbours_untouched(dbuf) and neighbours_untouched(qkvbuf) and neighbours_untouched(gbuf) and neighbours_untouched(obuf)
    assert torch.equal(qd.double().cpu(), inp["q_dev"]) and torch.equal(kd.double().cpu(), inp["k"])      # and the inputs are as they were
    assert torch.equal(vd.double().cpu(), inp["v"]) and torch.equal(dod.double().cpu(), inp["do"])
    assert torch.equal(tab, before) and torch.equal(tab.cpu(), tab_cpu if tab.dim() == 4 else tab_cpu[0])
