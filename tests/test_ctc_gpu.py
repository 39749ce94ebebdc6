"""CTC on the MI355X (csrc/ctc.hip) against the float64 restatement tests/ctc_ref.py, on the cases of tests/ctc_cases.py.

The tolerance is not fixed beforehand: for each case the error of torch's own fp32 CPU F.ctc_loss against float64 on the same inputs is
measured, the kernel gets 4 x that (a different but equally valid order of the sums), with a floor of 8 * 2^-24 * max(1, |nll|) for the
cases where torch happens to be exact; a bf16 d-logits output gets 2^-8 relative for its rounding in addition.  Both errors are printed
(profiles/ctc_loss.md records them)."""
import functools

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from tests import ctc_cases as CC
from tests import ctc_ref as R

pytestmark = pytest.mark.gpu

PARITY = ["a", "b31", "b32", "c", "d", "d_bf16", "e"]
FLOOR = 8.0 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def refs(key):
    """-> (case, logits fp32 as the kernel sees them (bf16-rounded for the bf16 case), float64 reference with zero_infinity, tol_nll,
    tol_unit, torch's fp32 errors): computed once, shared, read-only"""
    name, bf16 = (key[:-5], True) if key.endswith("_bf16") else (key, False)
    return refs_of(CC.make(name), bf16)


def refs_of(case, bf16):
    x = case["logits"].to(torch.bfloat16).float() if bf16 else case["logits"]
    ref = R.ctc(x.numpy(), case["targets"].numpy(), case["input_lengths"].numpy(), case["target_lengths"].numpy(), blank=case["blank"],
                zero_infinity=True, want_lattice=True)
    assert int(np.isinf(ref["raw"]).sum()) == case["infeasible"]
    nll32, grad32 = CC.torch_ctc(case, torch.float32, "none", True, logits=x)
    err_nll = float(np.abs(nll32.numpy().astype(np.float64) - ref["nll"]).max())
    err_unit = float(np.abs(grad32.numpy().astype(np.float64) - ref["unit"]).max())
    scale = max(1.0, float(np.abs(ref["nll"]).max()))
    return case, x, ref, max(4.0 * err_nll, FLOOR * scale), max(4.0 * err_unit, FLOOR * scale), (err_nll, err_unit)


def on_gpu(case, x, dtype=torch.float32):
    """the case on the device, the logits with the case's row stride (NaN in the padding)"""
    B, T, C = x.shape
    store = torch.full((B, T, case["ld"]), float("nan"), dtype=dtype, device="cuda")
    store[:, :, :C] = x.to(dtype).cuda()
    return store[:, :, :C], case["targets"].cuda(), case["input_lengths"].cuda(), case["target_lengths"].cuda()


def padded_out(case, shape, dtype):
    B, T, C = shape
    store = torch.full((B, T, case["ld"]), float("nan"), dtype=dtype, device="cuda")
    return store, store[:, :, :C]


def gout_for(reduction, B):
    if reduction == "none":
        return torch.tensor([0.5 + 0.25 * b for b in range(B)], dtype=torch.float32)
    return torch.tensor([0.5], dtype=torch.float32)


def factor(ref, reduction, gout):
    """per-sample |g_b| with the reduction's own factor"""
    B = len(ref["nll"])
    g = np.broadcast_to(gout.numpy().astype(np.float64), (B,)).copy()
    return np.abs(g / (B * np.maximum(ref["Lb"], 1)) if reduction == "mean" else g)


@pytest.mark.parametrize("key", PARITY)
def test_parity_with_float64(key):
    case, x, ref, tol_nll, tol_unit, (err_nll, err_unit) = refs(key)
    dtype = torch.bfloat16 if key.endswith("_bf16") else torch.float32
    lg, tg, il, tl = on_gpu(case, x, dtype)
    B, T, C = x.shape
    assert K.ctc_route(tg.shape[1]) == (K._lib.CTC_WAVE if 2 * tg.shape[1] + 1 <= 64 else K._lib.CTC_LDS)
    for reduction in ("none", "sum", "mean"):
        st = K.ctc_loss_fwd(lg, tg, il, tl, case["blank"], reduction, True)
        nll = st.nll.cpu().numpy().astype(np.float64)
        k_nll = float(np.abs(nll - ref["nll"]).max())
        want = float(np.sum(R.reduce(ref["nll"], ref["Lb"], reduction if reduction != "none" else "sum")))
        # the reduced loss: the per-sample bound through the reduction (a sum of B terms, or their mean over >= 1 label each)
        tol_red = tol_nll * (1.0 if reduction == "mean" else B)
        k_red = abs(float(st.loss2[0]) - want)
        assert float(st.loss2[1]) == B
        gout = gout_for(reduction, B)
        store, dl = padded_out(case, x.shape, dtype)
        K.ctc_loss_bwd(lg, st, gout.cuda(), dl)
        got = dl.float().cpu().numpy().astype(np.float64)
        want_dl = R.dlogits(ref, reduction, gout.numpy())
        f = factor(ref, reduction, gout)
        bound = tol_unit * f[:, None, None] + (2.0 ** -8 * np.abs(want_dl) if dtype == torch.bfloat16 else 0.0)
        k_unit = float((np.abs(got - want_dl) / np.maximum(f, 1e-300)[:, None, None]).max())
        print(f"ctc parity {key:7s} {reduction:4s}: nll |torch fp32 - f64| {err_nll:.3e}  |kernel - f64| {k_nll:.3e} (tol {tol_nll:.3e});  "
              f"dlogits/g |torch fp32 - f64| {err_unit:.3e}  |kernel - f64| {k_unit:.3e} (tol {tol_unit:.3e});  max |nll| {np.abs(ref['nll']).max():.1f}")
        assert k_nll <= tol_nll, (key, reduction, k_nll, tol_nll)
        assert k_red <= tol_red, (key, reduction, k_red, tol_red)
        assert np.all(np.abs(got - want_dl) <= bound), (key, reduction, k_unit, tol_unit)
        # exact statements: frames past the sample's end and samples without alignment are 0.0; the row padding keeps its poison
        for b in range(B):
            assert not got[b, int(ref["Tb"][b]):].any()
            if np.isinf(ref["raw"][b]):
                assert nll[b] == 0.0 and not got[b].any()
        if case["ld"] > C:
            assert bool(torch.isnan(store[:, :, C:]).all())


@functools.lru_cache(maxsize=None)
def misaligned_case():
    """B = 2, T = 5, C = 13, Lmax = 3: contiguous logits (row stride 13), one adjacent repeat, a sample that ends early"""
    g = torch.Generator().manual_seed(1313)
    return dict(name="misaligned", logits=3.0 * torch.randn((2, 5, 13), generator=g), targets=torch.tensor([[4, 4, 9], [12, 1, CC.PAD]]),
                input_lengths=torch.tensor([5, 3]), target_lengths=torch.tensor([3, 2]), blank=0, infeasible=0, ld=13)


@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_rows_that_disagree_about_the_vector_boundary(dtype, reduction):
    """logits rows at stride 13 from an aligned base, dlogits rows at stride 16 from one element into its storage: on most rows the two
    pointers reach their first 16-byte boundary after a different number of elements and ctc_bwd_kernel goes element by element"""
    case = misaligned_case()
    _, x, ref, _, tol_unit, _ = refs_of(case, dtype == torch.bfloat16)
    B, T, C = x.shape
    lg = x.to(dtype).cuda()
    assert lg.is_contiguous() and lg.stride(1) == C
    store = torch.full((1 + B * T * 16 + 7,), float("nan"), dtype=dtype, device="cuda")
    dl = store[1:1 + B * T * 16].view(B, T, 16)[:, :, :C]
    per_vec = 16 // lg.element_size()
    heads = [[(-(p.data_ptr() // p.element_size())) % per_vec for p in (lg[b, t], dl[b, t])] for b in range(B) for t in range(T)]
    assert sum(hl != hd for hl, hd in heads) > B * T // 2
    st = K.ctc_loss_fwd(lg, case["targets"].cuda(), case["input_lengths"].cuda(), case["target_lengths"].cuda(), 0, reduction, True)
    gout = gout_for(reduction, B)
    K.ctc_loss_bwd(lg, st, gout.cuda(), dl)
    got = dl.float().cpu().numpy().astype(np.float64)
    want = R.dlogits(ref, reduction, gout.numpy())
    f = factor(ref, reduction, gout)
    bound = tol_unit * f[:, None, None] + (2.0 ** -8 * np.abs(want) if dtype == torch.bfloat16 else 0.0)
    k_unit = float((np.abs(got - want) / f[:, None, None]).max())
    print(f"ctc misaligned backward {dtype} {reduction}: dlogits/g |kernel - f64| {k_unit:.3e} (tol {tol_unit:.3e})")
    assert np.all(np.abs(got - want) <= bound), (k_unit, tol_unit)
    inside = torch.zeros(store.numel(), dtype=torch.bool, device="cuda")
    inside[1:1 + B * T * 16].view(B, T, 16)[:, :, :C] = True
    assert bool(torch.isnan(store[~inside]).all()) and not bool(torch.isnan(store[inside]).any())
    for b in range(B):
        assert not got[b, int(ref["Tb"][b]):].any()


@pytest.mark.parametrize("key", ["a", "b31", "b32", "c", "d"])
def test_lattice_sums_to_the_loss_at_every_frame(key):
    """-logsumexp_s(alpha_t(s) + beta_t(s) - lp_t(l'_s)) = nll_b at EVERY t < T_b: a wrong step anywhere in either chain shows, not only
    one at the end"""
    case, x, ref, tol_nll, _, _ = refs(key)
    lg, tg, il, tl = on_gpu(case, x)
    st = K.ctc_loss_fwd(lg, tg, il, tl, case["blank"], "none", True, want_grad=False, want_lattice=True)
    alpha, beta = st.alpha.cpu().numpy().astype(np.float64), st.beta.cpu().numpy().astype(np.float64)
    lp = x.numpy().astype(np.float64) - st.row_lse.cpu().numpy().astype(np.float64)[..., None]
    # row_lse: the rounding of the result and of the exponentials, plus a lane's chain of at most C / 64 fp32 additions
    np.testing.assert_allclose(st.row_lse.cpu().numpy(), ref["lse"], rtol=0, atol=2.0 ** -24 * (np.abs(ref["lse"]).max() + 4 + x.shape[2] / 64))
    worst = 0.0
    for b in range(x.shape[0]):
        if np.isinf(ref["raw"][b]):
            continue
        tb, S = int(ref["Tb"][b]), 2 * int(ref["Lb"][b]) + 1
        ext = R.extended(case["targets"][b, :ref["Lb"][b]].numpy(), case["blank"])
        tot = -R.logsumexp(alpha[b, :tb, :S] + beta[b, :tb, :S] - lp[b, :tb][:, ext], axis=1)
        worst = max(worst, float(np.abs(tot - ref["nll"][b]).max()))
        assert np.all(np.isneginf(alpha[b, :tb, S:])) and np.all(np.isneginf(beta[b, :tb, S:]))
    print(f"ctc lattice {key}: worst |frame total - nll| {worst:.3e} (tol {tol_nll:.3e})")
    assert worst <= tol_nll


def test_single_alignment_is_the_sum_along_it():
    case, x, ref, tol_nll, _, _ = refs("a")
    lg, tg, il, tl = on_gpu(case, x)
    st = K.ctc_loss_fwd(lg, tg, il, tl, 0, "none", False, want_grad=False)
    path = [2, 0, 2, 3, 0, 3]
    want = -sum(ref["lp"][2, t, c] for t, c in enumerate(path))
    assert abs(float(st.nll[2]) - want) <= tol_nll


def _run(lg, tg, il, tl, blank, reduction, zero_infinity, gout):
    st = K.ctc_loss_fwd(lg, tg, il, tl, blank, reduction, zero_infinity)
    dl = K.ctc_loss_bwd(lg, st, gout)
    return st.nll.clone(), st.loss2.clone(), dl


@pytest.mark.parametrize("key", ["d", "e", "b32"])
def test_exact_statements(key):
    case, x, ref, _, _, _ = refs(key)
    lg, tg, il, tl = on_gpu(case, x)
    B = x.shape[0]
    g = gout_for("mean", B).cuda()
    nll1, loss1, dl1 = _run(lg, tg, il, tl, case["blank"], "mean", True, g)
    # two runs: the same bits
    nll2, loss2, dl2 = _run(lg, tg, il, tl, case["blank"], "mean", True, g)
    assert torch.equal(nll1, nll2) and torch.equal(loss1, loss2) and torch.equal(dl1, dl2)
    assert bool(torch.isfinite(dl1).all())
    # padded targets without explicit lengths: the same bits
    nll3, loss3, dl3 = _run(lg, tg, il, None, case["blank"], "mean", True, g)
    assert torch.equal(nll1, nll3) and torch.equal(loss1, loss3) and torch.equal(dl1, dl3)
    # zero_infinity off: +inf where no alignment exists, every other sample unchanged bit for bit
    nll4, _, dl4 = _run(lg, tg, il, tl, case["blank"], "mean", False, g)
    inf = torch.from_numpy(np.isinf(ref["raw"])).cuda()
    assert int(inf.sum()) == case["infeasible"]
    assert bool(torch.isposinf(nll4[inf]).all()) and bool((nll1[inf] == 0.0).all()) and torch.equal(nll4[~inf], nll1[~inf])
    assert torch.equal(dl4[~inf], dl1[~inf]) and not bool(dl1[inf].any())


@pytest.mark.parametrize("key", ["a", "b32"])
def test_clamps_keep_every_access_inside(key):
    """a label past the classes, a label equal to the blank, lengths past the buffers: the calls return (the result is meaningless) and
    the guard bands around every buffer stay intact (the autouse fixture checks them)"""
    case, x, _, _, _, _ = refs(key)
    lg, tg, il, tl = on_gpu(case, x)
    B, T, C = x.shape
    tg = tg.clone()
    tg[0, 0], tg[0, 1], tg[B - 1, 0] = C + 7, case["blank"], -5
    il, tl = il.clone(), tl.clone()
    il[0], tl[0], il[B - 1] = T + 5, tg.shape[1] + 3, -2
    for tlen in (tl, None):
        st = K.ctc_loss_fwd(lg, tg, il, tlen, case["blank"], "sum", True, want_lattice=True)
        dl = K.ctc_loss_bwd(lg, st, torch.ones(1, device="cuda"))
        ids, lens = E.ctc_greedy_decode(lg.contiguous(), il, blank=case["blank"])
        torch.cuda.synchronize()
        assert dl.shape == lg.shape and int(lens.max()) <= T and int(lens[B - 1]) == 0


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_autograd(reduction):
    case, x, ref, _, tol_unit, _ = refs("b32")
    lg, tg, il, tl = on_gpu(case, x)
    B = x.shape[0]
    leaf = lg.contiguous().requires_grad_(True)
    loss = E.ctc_loss(leaf, tg, il, tl, blank=case["blank"], reduction=reduction, zero_infinity=True)
    if reduction == "none":
        w = gout_for("none", B)
        assert loss.shape == (B,)
        loss.backward(w.cuda())
    else:
        w = torch.tensor([0.5])
        assert loss.dim() == 0
        loss.mul(0.5).backward()
    want = R.dlogits(ref, reduction, w.numpy())
    f = factor(ref, reduction, w)
    assert np.all(np.abs(leaf.grad.cpu().numpy().astype(np.float64) - want) <= tol_unit * f[:, None, None])
    with torch.no_grad():                                 # no gradient wanted: the alpha recursion alone, the same loss
        loss2 = E.ctc_loss(leaf, tg, il, tl, blank=case["blank"], reduction=reduction, zero_infinity=True)
    assert torch.equal(loss2, loss.detach())


def test_no_host_synchronisation():
    """loss, backward and greedy decoding inside a stream capture (which raises on anything that waits for the host), padded targets
    counted on the device; the replay gives the eager bits"""
    case, x, _, _, _, _ = refs("a")
    lg, tg, il, _ = on_gpu(case, x)
    leaf = lg.contiguous().requires_grad_(True)

    def step():
        loss = E.ctc_loss(leaf, tg, il, None, blank=0, reduction="mean", zero_infinity=True)
        loss.backward()
        return loss.detach(), E.ctc_greedy_decode(leaf.detach(), il, blank=0)

    loss0, (ids0, len0) = step()
    grad0 = leaf.grad.clone()
    leaf.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    leaf.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss1, (ids1, len1) = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss0) and torch.equal(leaf.grad, grad0) and torch.equal(ids1, ids0) and torch.equal(len1, len0)


def test_collapse():
    _, A, B_ = 0, 1, 2
    T = 70
    g = torch.Generator().manual_seed(5)
    rows = [([A, A, _, A, B_, B_] * 12)[:T], torch.randint(0, 4, (T,), generator=g).tolist(), [B_] * T]
    am = torch.tensor(rows, dtype=torch.int64)
    for il in (None, torch.tensor([3, 65, 70]), torch.tensor([0, 70, 1])):
        ids, lens = K.ctc_collapse(am.cuda(), None if il is None else il.cuda(), blank=0, pad=-100)
        want_ids, want_lens = R.collapse(am.numpy(), None if il is None else il.numpy(), blank=0, pad=-100)
        assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(lens.cpu().numpy(), want_lens)
    for frames, want in (([_, _, _], []), ([A, _, A], [A, A]), ([A, A, _], [A])):
        row = torch.tensor([frames + [_] * (T - 3)] * 3, dtype=torch.int64)
        ids, lens = K.ctc_collapse(row.cuda(), blank=0, pad=-7)
        assert lens.tolist() == [len(want)] * 3 and ids[1, :len(want)].tolist() == want and bool((ids[:, len(want):] == -7).all())
    # more frames than one pass of the workgroup, another blank
    am = torch.randint(0, 3, (3, 300), generator=g)
    ids, lens = K.ctc_collapse(am.cuda(), torch.tensor([300, 257, 256]).cuda(), blank=2, pad=-100)
    want_ids, want_lens = R.collapse(am.numpy(), [300, 257, 256], blank=2, pad=-100)
    assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(lens.cpu().numpy(), want_lens)


# ---- model ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def _model_cfg():
    from frankenstein_amd.models import brainformer as bf
    enc = bf.MAEConfig(window_size=200, n_electrodes=64, patch_size=25, dim=128, n_layers=2, head_dim=32, hidden_dim=512, n_heads=4, n_kv_heads=4)
    return bf.Config(encoder=enc, n_output_tokens=8, output_dim=6, dim=128, n_layers=1, head_dim=32, hidden_dim=256, n_heads=4, n_kv_heads=4)


def _grads(m):
    return {k: p.grad.detach().float().cpu().numpy().copy() for k, p in m.named_parameters() if p.grad is not None}


def test_model_loss_gradients_and_decoding(fp32_mode):
    from frankenstein_amd.models.notebook_models import BrainFormerCTC
    torch.manual_seed(3)
    m = BrainFormerCTC(_model_cfg()).cuda()
    assert m.blank == 5
    with torch.no_grad():                                 # a head that does not start at zero, so that the frames differ
        m.perceiver["to_words"].weight.normal_(0.0, 0.5)
    x = torch.randn(2, 200, 64, device="cuda")
    targets = torch.tensor([[1, 1, 2, -100], [3, 0, 4, 2]], device="cuda")
    loss, logits = m(x, targets)
    assert logits.shape == (2, 8, 6)
    ref = R.ctc(logits.detach().float().cpu().numpy(), targets.cpu().numpy(), blank=5, zero_infinity=True)
    assert np.isfinite(ref["raw"]).all()
    assert abs(float(loss.detach()) - float(R.reduce(ref["nll"], ref["Lb"], "mean"))) < 1e-5
    loss.backward()
    got = _grads(m)
    m.zero_grad(set_to_none=True)
    # the kernels are the same either side of the loss: the reference d-logits pushed through the same backward
    m.features(x).backward(torch.from_numpy(R.dlogits(ref, "mean", 1.0)).to(logits.dtype).cuda())
    want = _grads(m)
    assert got.keys() == want.keys() and len(got) > 10
    for k in got:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-3, atol=2e-5, err_msg=k)
    ids, lens = m.decode(x)
    want_ids, want_lens = R.collapse(logits.detach().float().cpu().numpy().argmax(-1), blank=5, pad=-100)
    assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(lens.cpu().numpy(), want_lens)
    none_loss, logits2 = m(x)
    assert none_loss is None and torch.equal(logits2, logits)
    # a sentence longer than the read-out does not turn the loss into inf: it contributes 0
    long = torch.tensor([[1, 1, 2] + [-100] * 7, [0, 1, 2, 3, 4, 0, 1, 2, 3, 4]], device="cuda")
    loss_long, _ = m(x, long)
    assert abs(float(loss_long.detach()) - float(ref["nll"][0]) / 3 / 2) < 1e-5


def test_model_graphed_step_equals_eager(fp32_mode):
    """three GraphedTrainStep replays against three eager train_step calls: the same losses and the same parameters bit for bit"""
    from frankenstein_amd.models.notebook_models import BrainFormerCTC
    from frankenstein_amd.utils import train_utils as tu
    cfg = _model_cfg()
    g = torch.Generator(device="cuda").manual_seed(11)
    tgt = torch.tensor([[1, 1, 2, -100], [3, 0, 4, 2]], device="cuda")
    batches = [(torch.randn(2, 200, 64, device="cuda", generator=g), tgt.roll(i, 0), None) for i in range(3)]
    tc = tu.TrainConfig(mixed_precision=False, use_scheduler=True, learning_rate=1e-3, warmup_iters=2, max_steps=10, lr_decay_iters=10)
    runs = []
    try:
        for graphed in (False, True):
            torch.manual_seed(0)
            m = BrainFormerCTC(cfg).cuda()
            opt = tu.FusedAdamW(m, lr=1e-3, weight_decay=1e-2, grad_clip=1.0)
            if graphed:
                step = tu.GraphedTrainStep(m, batches[0], opt, tc)
                losses = [float(step(b, i)) for i, b in enumerate(batches)]
            else:
                losses = [float(tu.train_step(m, b, opt, i, tc)) for i, b in enumerate(batches)]
            assert opt.t == 3 and all(np.isfinite(losses))
            runs.append((losses, opt.arena.flat.detach().clone(), opt.m.clone()))
        assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
        assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    finally:
        E.enable_wgrad_stream(False)
