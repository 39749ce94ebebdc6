"""attn_fwd and attn_bwd with a dropout tuple (fk_attn_fwd_dropout / fk_attn_bwd_dropout, the training path of the GPT decoder): every keep
decision of every kernel, against a float64 reference that takes the decisions from the host (tests/dropout_ref.py).  No mask is stored:
the forward, the dQ and the dK/dV kernel of csrc/attention.hip each rebuild keep / drop from (b, h, row, key) with index arithmetic of their
own, and under dropout the backward kernels run their per-element path on every tile.  If the three disagree the forward looks fine and
dq, dk and dv are silently wrong; the inputs of tests/attn_inputs.py make one wrong decision an error of many times the bound
(tests/test_attn_drop_cpu.py proves that on the reference alone, for every case, every kind of wrong mask, and single bits in every tile
pair and at every residue mod 64).

Each case (tests/cases.py ATTN_DROP_CASES; the CPU file pins the routes and what the list covers): layout "split" = q in its own buffer,
k | v side by side, dq alone and dk | dv side by side; layout "qkv" = q | k | v the three views of one sentinel-filled
[B, N, 3 H D + 2 PAD] buffer and dq | dk | dv those of a second one, as engine.AttnBranch passes them; o and dO in guarded buffers of their
own with equal strides.  The route is asked of attn_route_names(..., dropout=True) before the launch; attn_fwd(dropout=(p, words, site)),
then attn_bwd with the same tuple (and rope_table on the RoPE cases) on the forward's o and lse.  o, dq, dk and dv are compared on every
element,
    |got - ref| <= [2^-8 |ref| + 2^-8 mag, bf16 only] + 2e-5 + 2e-5 mag          lse: atol = rtol = 1e-4
with Pd = P * keep / (1 - p) in the last products and in mag (derivation: tests/attn_inputs.py); lse is bit-equal to the undropped
forward's, +inf exactly on the fully masked rows; the sentinels beside every view stay and the inputs and the seed words are unchanged.
Prints "FRAC <tensor> <routes> <largest error / bound>".

FRAC maxima over the cases on the MI355X (every case passes), beside the CPU rounding model's (tests/test_attn_drop_cpu.py):
             o      dq     dk     dv     lse
  MI355X     0.82   0.81   0.89   0.93   0.0010
  CPU model  0.84   0.81   0.89   0.94"""
import pytest
import torch

from tests import attn_inputs as AI
from tests import cases
from tests.test_attn_routes_gpu import check, guarded, neighbours_untouched
from tests.test_attn_rope_gpu import device_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def seed_words(seed, step):
    return torch.tensor([seed, step], dtype=torch.int32, device="cuda")


class Problem:
    """the device buffers of a case in its layout, filled with the reference's operands"""

    def __init__(self, K, case):
        B, H, Nq, Nk, D = case["B"], case["H"], case["Nq"], case["Nk"], case["D"]
        self.case, self.inp = case, AI.make_inputs(case)
        inp = self.inp
        self.dtype = dtype = inp["dtype"]
        self.mask = AI.make_mask(K, case, inp["extras"], inp["vis"], "cuda")
        self.routes = K.attn_route_names(Nq, Nk, D, dtype, self.mask, dropout=True, rope="table" in case)
        assert self.routes == case["routes"] == ("FWD_GENERIC", "DQ_GENERIC", "DKDV_GENERIC"), f"{case['id']} reaches {self.routes}"
        if case["layout"] == "qkv":
            buf, (self.q, self.k, self.v) = guarded(B, Nq, H, D, dtype, parts=3)
            self.in_bufs = [buf]
        else:
            qbuf, (self.q,) = guarded(B, Nq, H, D, dtype)
            kvbuf, (self.k, self.v) = guarded(B, Nk, H, D, dtype, parts=2)
            self.in_bufs = [qbuf, kvbuf]
        gbuf, (self.do,) = guarded(B, Nq, H, D, dtype)
        self.in_bufs.append(gbuf)
        for dst, src in ((self.q, inp["q_dev"]), (self.k, inp["k"]), (self.v, inp["v"]), (self.do, inp["do"])):
            dst.copy_(src.to(dtype))
            assert torch.equal(dst.double().cpu(), src)                        # the device holds the reference's operand values
        self.ops = tuple(AI.heads(inp[n]) for n in ("q", "k", "v", "do"))

    def outputs(self):
        """-> (buffers, o, dq, dk, dv): fresh sentinel-filled outputs in the case's layout"""
        c = self.case
        B, H, Nq, Nk, D = c["B"], c["H"], c["Nq"], c["Nk"], c["D"]
        obuf, (o,) = guarded(B, Nq, H, D, self.dtype)
        if c["layout"] == "qkv":
            dbuf, (dq, dk, dv) = guarded(B, Nq, H, D, self.dtype, parts=3)
            return [obuf, dbuf], o, dq, dk, dv
        dqbuf, (dq,) = guarded(B, Nq, H, D, self.dtype)
        dkvbuf, (dk, dv) = guarded(B, Nk, H, D, self.dtype, parts=2)
        return [obuf, dqbuf, dkvbuf], o, dq, dk, dv

    def inputs_unchanged(self):
        inp = self.inp
        return (all(neighbours_untouched(b) for b in self.in_bufs) and torch.equal(self.q.double().cpu(), inp["q_dev"])
                and torch.equal(self.k.double().cpu(), inp["k"]) and torch.equal(self.v.double().cpu(), inp["v"])
                and torch.equal(self.do.double().cpu(), inp["do"]))


def check_lse(routes, lse, lref):
    lse_c = lse.double().cpu()
    dead = torch.isinf(lref)
    assert torch.equal(torch.isinf(lse_c) & (lse_c > 0), dead), "fully masked rows: lse = +inf, and only there"
    lerr = ((lse_c - lref)[~dead].abs() / (1e-4 + 1e-4 * lref[~dead].abs())).max()
    print(f"FRAC lse {'.'.join(routes)} {float(lerr):.4f}")
    assert float(lerr) <= 1.0


def run_case(K, case, dropout=True):
    """dropout=False: the same launches with dropout=None against the reference with keep = 1 (the evaluation path)"""
    pr = Problem(K, case)
    inp, dtype, routes, scale, vis = pr.inp, pr.dtype, pr.routes, pr.inp["scale"], pr.inp["vis"]
    q, k, v, do = pr.ops
    if dropout:
        words = seed_words(case["seed"], case["step"])
        drop = (case["p"], words, case["site"])
        keep, s = AI.case_keep(case), AI.drop_scale32(case["p"])
    else:
        words, drop = None, None
        assert K.attn_route_names(case["Nq"], case["Nk"], case["D"], dtype, pr.mask) == routes
        keep, s = torch.ones(case["B"], case["H"], case["Nq"], case["Nk"], dtype=torch.bool), 1.0
    bufs, o, dq, dk, dv = pr.outputs()
    _, lse = K.attn_fwd(pr.q, pr.k, pr.v, pr.mask, scale=scale, out=o, dropout=drop)
    oref, lref, mag_o, P = AI.forward(q, k, v, vis, scale, keep, s)
    check("o", routes, o, oref, mag_o, dtype)
    check_lse(routes, lse, lref)
    if dropout:
        _, lse0 = K.attn_fwd(pr.q, pr.k, pr.v, pr.mask, scale=scale)
        assert torch.equal(lse.view(torch.int32), lse0.view(torch.int32))      # the softmax statistics do not see the dropout

    kw = {}
    if "table" in case:
        tab, tab_cpu = device_table(case)
        before = tab.clone()
        kw = dict(rope_table=tab, rope_off=case["rope_off"])
    K.attn_bwd(pr.q, pr.k, pr.v, o, pr.do, lse, dq, dk, dv, pr.mask, scale=scale, dropout=drop, **kw)
    ref = AI.backward(q, k, v, do, P, AI.heads(o.double().cpu()), scale, keep, s)
    if "table" in case:
        ref = AI.unrotate_grads(ref, tab_cpu, case["rope_off"])
        assert torch.equal(tab, before)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        check(name, routes, got, ref[name], ref["mag_" + name], dtype)
    assert all(neighbours_untouched(b) for b in bufs) and pr.inputs_unchanged()
    if dropout:
        assert words.tolist() == [case["seed"], case["step"]]


@pytest.mark.parametrize("case", cases.ATTN_DROP_CASES, ids=lambda c: c["id"])
def test_attention_dropout_against_float64(K, case):
    run_case(K, case)


def test_without_a_dropout_tuple_the_reference_with_every_key_kept_holds(K):
    """dropout=None on one of the cases (the engine's call, bf16) equals forward / backward with keep = 1, drop_scale = 1: the optional
    arguments of the extended reference change nothing when nothing is dropped"""
    case = next(c for c in cases.ATTN_DROP_CASES if c["layout"] == "qkv" and c["dtype"] == "bf16" and "table" not in c)
    run_case(K, case, dropout=False)


def test_a_captured_step_draws_the_mask_of_the_step_word_on_every_replay(K):
    """One forward + backward with dropout captured in a graph; the step word lives on the device, so adding 1 to it between two replays
    gives the second replay another mask.  Each replay's o, lse, dq, dk, dv are bit-equal to an eager run with that step word, each o
    holds its bound against the host's prediction for that step, and the two replays differ."""
    case = cases.ATTN_DROP_GRAPH_CASE
    pr = Problem(K, case)
    scale, p, site, seed, step = pr.inp["scale"], case["p"], case["site"], case["seed"], case["step"]
    q, k, v, do = pr.ops

    def launch(words, o, dq, dk, dv):
        _, lse = K.attn_fwd(pr.q, pr.k, pr.v, pr.mask, scale=scale, out=o, dropout=(p, words, site))
        K.attn_bwd(pr.q, pr.k, pr.v, o, pr.do, lse, dq, dk, dv, pr.mask, scale=scale, dropout=(p, words, site))
        return lse

    eager = []
    for n in (0, 1):
        _, o, dq, dk, dv = pr.outputs()
        lse = launch(seed_words(seed, step + n), o, dq, dk, dv)
        eager.append([t.clone() for t in (o, lse, dq, dk, dv)])
    torch.cuda.synchronize()

    words = seed_words(seed, step)
    bufs, o, dq, dk, dv = pr.outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up: the allocator
        launch(words, o, dq, dk, dv)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lse = launch(words, o, dq, dk, dv)
    seen = []
    for n in (0, 1):
        g.replay()
        torch.cuda.synchronize()
        assert words.tolist() == [seed, step + n]
        got = [t.clone() for t in (o, lse, dq, dk, dv)]
        for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, eager[n]):
            assert torch.equal(a, b), f"replay {n}: {name} differs from the eager run with step word {step + n}"
        oref, _, mag_o, _ = AI.forward(q, k, v, pr.inp["vis"], scale, AI.case_keep(case, step=step + n), AI.drop_scale32(p))
        check(f"o replay {n}", pr.routes, o, oref, mag_o, pr.dtype)
        seen.append(got)
        words[1:].add_(1)
    for i in (0, 2, 3, 4):
        assert not torch.equal(seen[0][i], seen[1][i])
    assert torch.equal(seen[0][1], seen[1][1])                                 # lse does not see the dropout
    assert all(neighbours_untouched(b) for b in bufs) and pr.inputs_unchanged()
