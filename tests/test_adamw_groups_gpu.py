"""fk_adamw_step_groups / fk_grad_sumsq and the grouped FusedAdamW on the GPU.

References: oracle.ref_train.adamw_step / clip_grad_value in float64, torch.optim.AdamW and torch.nn.utils.clip_grad_norm_ on float64
CPU copies.  Element bounds: the ones tests/test_rowwise_gpu.py::adamw_check holds this arithmetic to (rtol 2e-6; atol 2e-7 for p and
m, 1e-9 for v).  A multi-step comparison restarts the reference from the device's previous state at every step, so the one-step bound
applies unchanged.  The norm clip multiplies the gradient by an fp32 coefficient whose relative error (an fp32 sum of squares in a
fixed tree order, one square root, one division: < 1e-6) stays inside the same bounds because the inputs keep |gradient| of order 1."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import ref_train as RT
from tests import cases as C

pytestmark = pytest.mark.gpu

BIG = 4 * 4096 * 256 + 1200               # past one pass of the 4096-block grid, ends inside a block
RTOL, ATOL_PM, ATOL_V = 2e-6, 2e-7, 1e-9
SLOTS3 = [(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1), (3e-4, 0.8, 0.95, 1e-6, 0.0, 3), (2e-3, 0.95, 0.99, 1e-10, 0.1, 1000)]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    import frankenstein_amd as fa
    fa.set_compute_dtype("bf16")


def rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def state(n, seed=1, gscale=1.0):
    """p, g, m, v on the host (fp32): |g| of order 1, moments as after a few steps"""
    return rnd(n, seed), rnd(n, seed + 1, gscale), rnd(n, seed + 2, 0.1), rnd(n, seed + 3, 0.1).abs()


def ref_update(p, g, m, v, seg, hyper, clip=0.0, gscale=1.0, coef=1.0):
    """float64 AdamW of one segment from fp32 inputs: the effective gradient is g * gscale * coef, value-clipped if clip > 0"""
    b, e, _ = seg
    lr, b1, b2, eps, wd, step = hyper
    geff = g[b:e].double() * gscale * coef
    if clip > 0:
        geff = RT.clip_grad_value(geff, clip)
    return RT.adamw_step(p[b:e].double(), geff, m[b:e].double(), v[b:e].double(), step, lr, wd, b1, b2, eps)


def check_segments(host, devs, segs, slots, clip, gscale, zero_grad, coef=1.0):
    """every segment within the element bounds of its float64 update, its gradient zeroed; every other element bit-unchanged"""
    p0, g0, m0, v0 = host
    pd, gd, md, vd = (t.cpu() for t in devs)
    covered = torch.zeros(p0.numel(), dtype=torch.bool)
    for seg in segs:
        b, e, s = seg
        covered[b:e] = True
        pr, mr, vr = ref_update(p0, g0, m0, v0, seg, slots[s], clip, gscale, coef)
        for got, want, atol, what in ((pd, pr, ATOL_PM, "p"), (md, mr, ATOL_PM, "m"), (vd, vr, ATOL_V, "v")):
            torch.testing.assert_close(got[b:e], want.float(), rtol=RTOL, atol=atol, msg=lambda t: f"{what} of segment {seg}: {t}")
        if zero_grad:
            assert int(torch.count_nonzero(gd[b:e])) == 0, seg
        else:
            assert torch.equal(gd[b:e], g0[b:e]), seg
    out = ~covered
    for got, was, what in ((pd, p0, "p"), (gd, g0, "g"), (md, m0, "m"), (vd, v0, "v")):
        assert torch.equal(got[out], was[out]), f"{what} outside the segments changed"


def run_groups(K, host, segs, slots, **kw):
    devs = [t.clone().cuda() for t in host]
    K.adamw_step_groups_(*devs, K.adamw_segments(segs, "cuda"), slots, **kw)
    return devs


# =============================================================================================== 1, 2: segments against float64
def test_segments_slots_and_a_gap_against_float64(K):
    """segments of 4, 8, 1000 and 4*4096*256 + 1200 elements (the last one runs past one pass of the grid and ends inside a block), an
    8-element gap and 8 elements behind the last segment; three slots that differ in every hyper-parameter and in their step count"""
    segs = [(0, 4, 0), (4, 12, 1), (20, 1020, 2), (1020, 1020 + BIG, 1)]
    host = state(1020 + BIG + 8)
    devs = run_groups(K, host, segs, SLOTS3, clip=0.5, grad_scale=0.25, zero_grad=True)
    check_segments(host, devs, segs, SLOTS3, 0.5, 0.25, True)


@pytest.mark.parametrize("nseg", [1025, 3000])
def test_many_tiny_segments(K, nseg):
    """nseg segments of 4, 8 or 12 elements with alternating slots, a hole of 4 or 8 elements after every 37th: more segments than the
    1024 begins one LDS tile holds (the search finishes in the table itself: 2 or 3 records per staged begin), edges inside a wave"""
    rng = np.random.default_rng(nseg)
    segs, off = [], 0
    for i in range(nseg):
        n = int(rng.choice([4, 8, 12]))
        segs.append((off, off + n, i % 3))
        off += n + (int(rng.choice([4, 8])) if i % 37 == 36 else 0)
    host = state(off + 4, seed=7)
    devs = run_groups(K, host, segs, SLOTS3, clip=0.5, grad_scale=0.25, zero_grad=True)
    check_segments(host, devs, segs, SLOTS3, 0.5, 0.25, True)


# =============================================================================================== 3: the bits of fk_adamw_step
@pytest.mark.parametrize("n", [1004, BIG])
@pytest.mark.parametrize("clip,gscale,zero_grad", [(0.0, 1.0, False), (0.5, 0.25, True)])
def test_one_segment_one_slot_gives_the_bits_of_adamw_step(K, n, clip, gscale, zero_grad):
    host = state(n, seed=11)
    lr, b1, b2, eps, wd, step = 3e-4, 0.9, 0.999, 1e-8, 1e-2, 3
    want = [t.clone().cuda() for t in host]
    K.adamw_step_(*want, step, lr, b1, b2, eps, wd, clip=clip, grad_scale=gscale, zero_grad=zero_grad)
    got = run_groups(K, host, [(0, n, 0)], [(lr, b1, b2, eps, wd, step)], clip=clip, grad_scale=gscale, zero_grad=zero_grad)
    for a, b, what in zip(got, want, "pgmv"):
        assert torch.equal(a, b), what


# =============================================================================================== 4: the norm, exactly
def test_sumsq_is_exact_excludes_the_gap_and_repeats_its_bits(K):
    n_cov = 4 * 1024 * 256 + 36
    segs = [(0, 1000, 0), (1016, 16 + n_cov, 1)]
    n = 16 + n_cov + 8
    g = torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(3)).float()
    g[1000:1016] = 1000.0                               # the gap: not part of the norm
    g[16 + n_cov:] = -2000.0                            # behind the last segment: neither
    cov = torch.cat([g[b:e] for b, e, _ in segs]).numpy()
    exact = int((cov.astype(np.int64) ** 2).sum())
    assert exact < 2 ** 24 and float(np.cumsum(cov * cov, dtype=np.float32)[-1]) == exact       # every fp32 partial sum is an integer < 2^24
    tab, gd = K.adamw_segments(segs, "cuda"), g.cuda()
    part = K.grad_sumsq_(gd, tab)
    assert part.numel() == K.GRAD_SUMSQ_BLOCKS <= 1024
    assert float(part.double().sum()) == exact
    again = K.grad_sumsq_(gd, tab, torch.full_like(part, float("nan")))
    assert torch.equal(part, again)
    # the step kernel adds the partials itself: norm_out = grad_scale * sqrt(sumsq) in fp32
    p, _, m, v = (t.cuda() for t in state(n, seed=5))
    norm = torch.zeros(1, device="cuda")
    K.adamw_step_groups_(p, gd, m, v, tab, SLOTS3[:2], grad_scale=0.25, zero_grad=False, max_norm=1.0, partials=part, norm_out=norm)
    assert float(norm) == float(np.float32(0.25) * np.sqrt(np.float32(exact)))


# =============================================================================================== 5: the norm clip against torch
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_norm_clip_against_clip_grad_norm(K, gscale):
    segs = [(0, 40000, 0), (40008, 40008 + 70004, 1)]
    n = segs[-1][1] + 4
    host = state(n, seed=21, gscale=0.5)
    p0, g0, m0, v0 = host
    tab = K.adamw_segments(segs, "cuda")
    part = K.grad_sumsq_(g0.cuda(), tab)
    # torch's norm of the scaled gradient over the covered elements, float64
    ref_g = torch.nn.Parameter(torch.zeros(40000 + 70004, dtype=torch.float64))
    ref_g.grad = torch.cat([g0[b:e] for b, e, _ in segs]).double() * gscale
    total = float(torch.nn.utils.clip_grad_norm_([ref_g], 1e30))
    # max_norm above the norm: coefficient exactly 1, the bits of the call without a norm clip
    plain = run_groups(K, host, segs, SLOTS3[:2], grad_scale=gscale, zero_grad=True)
    norm = torch.zeros(1, device="cuda")
    above = run_groups(K, host, segs, SLOTS3[:2], grad_scale=gscale, zero_grad=True, max_norm=2.0 * total, partials=part, norm_out=norm)
    for a, b, what in zip(above, plain, "pgmv"):
        assert torch.equal(a, b), what
    np.testing.assert_allclose(float(norm), total, rtol=RTOL)
    # below: clip_grad_norm_ + AdamW in float64
    max_norm = 0.3 * total
    before = ref_g.grad.clone()
    torch.nn.utils.clip_grad_norm_([ref_g], max_norm)
    coef = max_norm / (total + 1e-6)                    # what clip_grad_norm_ has just multiplied the gradient by
    torch.testing.assert_close(ref_g.grad, before * coef, rtol=1e-14, atol=0.0)
    below = run_groups(K, host, segs, SLOTS3[:2], grad_scale=gscale, zero_grad=True, max_norm=max_norm, partials=part, norm_out=norm)
    check_segments(host, below, segs, SLOTS3[:2], 0.0, gscale, True, coef=coef)
    np.testing.assert_allclose(float(norm), total, rtol=RTOL)


# =============================================================================================== 6: the optimizer, no model kernels
class _Four(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(9)
        self.a = torch.nn.Parameter(torch.randn(3, generator=g))
        self.b = torch.nn.Parameter(torch.randn(5, 7, generator=g))
        self.c = torch.nn.Parameter(torch.randn(129, generator=g))
        self.d = torch.nn.Parameter(torch.randn(64, 64, generator=g))


def _four_groups(m):
    return [{'params': [m.b], 'weight_decay': 0.1}, {'params': [m.c], 'weight_decay': 0.0, 'lr_scale': 0.1, 'betas': (0.8, 0.95)}]


LRS = [1e-3, 2e-3, 5e-4, 1.5e-3, 1e-3]
NORM_CLIP = 30.0          # the gradients below have a norm of about 65, a tenth of that on step 3: clipped on four steps, not on one


def _four_grads(step):
    g = torch.Generator().manual_seed(100 + step)
    scale = 0.1 if step == 2 else 1.0
    return [torch.randn(s, generator=g) * scale for s in ((3,), (5, 7), (129,), (64, 64))]


def _set_lr(opt, lr):
    for g in opt.param_groups:
        g['lr'] = lr * g.get('lr_scale', 1.0)


def _four_step(tu_opt, step, reached):
    """write this step's gradients into the arena (rubbish where the parameter is not reached), declare them, step"""
    a = tu_opt.arena
    for i, (p, o, g) in enumerate(zip(a.params, a.offsets, _four_grads(step))):
        a.grad[o:o + p.numel()] = (g if reached[i] else torch.full_like(g, 77.0)).flatten().cuda()
    tu_opt.mark_touched(reached)
    _set_lr(tu_opt, LRS[step])
    tu_opt.step()


def _run_four(tu, mode, skip, resume_at=None):
    """five steps on the GPU -> per step (flat, m, v) on the host; mode "value": grad_clip 1.0, "norm": grad_clip_norm; skip: parameter
    c gets no gradient on steps 2 and 3; resume_at: after that many steps the run continues in a fresh model and optimizer that
    received the parameters and state_dict() of the first"""
    kw = dict(grad_clip=1.0) if mode == "value" else dict(grad_clip_norm=NORM_CLIP)
    m = _Four().cuda()
    opt = tu.FusedAdamW(m, lr=LRS[0], weight_decay=1e-2, param_groups=_four_groups(m), **kw)
    assert [len(g['params']) for g in opt.param_groups] == [1, 1, 2] and opt._group_of == [2, 0, 1, 2]
    out, norms = [], []
    for step in range(5):
        if step == resume_at:
            sd = copy.deepcopy(opt.state_dict())
            m2 = _Four().cuda()
            m2.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
            m, opt = m2, tu.FusedAdamW(m2, lr=123.0, weight_decay=0.5, param_groups=_four_groups(m2), **kw)
            opt.load_state_dict(sd)
        reached = [True, True, not (skip and step in (1, 2)), True]
        _four_step(opt, step, reached)
        out.append(tuple(t.detach().cpu().clone() for t in (opt.arena.flat, opt.m, opt.v)))
        norms.append(None if opt.last_grad_norm is None else float(opt.last_grad_norm))
        o = opt.arena.offsets[2]
        if not reached[2]:
            assert float(opt.arena.grad[o:o + 129].min()) == 77.0        # not reached: its gradient is not even zeroed
            opt.arena.grad[o:o + 129] = 0.0
        assert int(torch.count_nonzero(opt.arena.grad)) == 0
    return out, norms, opt


def _check_four_against_torch(tu, mode, skip):
    got, norms, opt = _run_four(tu, mode, skip)
    ref = _Four().double()
    rp = [ref.a, ref.b, ref.c, ref.d]
    ropt = torch.optim.AdamW([{'params': [ref.b], 'weight_decay': 0.1}, {'params': [ref.c], 'weight_decay': 0.0, 'betas': (0.8, 0.95)},
                              {'params': [ref.a, ref.d]}], lr=LRS[0], weight_decay=1e-2)
    scales = [1.0, 0.1, 1.0]
    offs, sizes = opt.arena.offsets, [p.numel() for p in rp]
    for step in range(5):
        if step > 0:                                    # restart the reference from the device's previous state
            flat, m_, v_ = got[step - 1]
            with torch.no_grad():
                for p, o, n in zip(rp, offs, sizes):
                    p.copy_(flat[o:o + n].view(p.shape).double())
                    if p in ropt.state:
                        ropt.state[p]['exp_avg'].copy_(m_[o:o + n].view(p.shape).double())
                        ropt.state[p]['exp_avg_sq'].copy_(v_[o:o + n].view(p.shape).double())
        for g, s in zip(ropt.param_groups, scales):
            g['lr'] = LRS[step] * s
        reached = [True, True, not (skip and step in (1, 2)), True]
        for p, g, r in zip(rp, _four_grads(step), reached):
            p.grad = g.double() if r else None
        if mode == "value":
            torch.nn.utils.clip_grad_value_(rp, 1.0)
        else:
            total = float(torch.nn.utils.clip_grad_norm_(rp, NORM_CLIP))
            np.testing.assert_allclose(norms[step], total, rtol=RTOL)
            assert (total > NORM_CLIP) == (step != 2)
        ropt.step()
        flat, m_, v_ = got[step]
        prev = got[step - 1] if step else None
        for i, (p, o, n) in enumerate(zip(rp, offs, sizes)):
            what = f"step {step} parameter {i}"
            torch.testing.assert_close(flat[o:o + n], p.detach().flatten().float(), rtol=RTOL, atol=ATOL_PM, msg=lambda t: f"p, {what}: {t}")
            if reached[i]:
                st = ropt.state[p]
                torch.testing.assert_close(m_[o:o + n], st['exp_avg'].flatten().float(), rtol=RTOL, atol=ATOL_PM, msg=lambda t: f"m, {what}: {t}")
                torch.testing.assert_close(v_[o:o + n], st['exp_avg_sq'].flatten().float(), rtol=RTOL, atol=ATOL_V, msg=lambda t: f"v, {what}: {t}")
            else:                                       # like torch's `grad is None`: no decay, no moment update -- not a bit moves
                for now, was in zip(got[step], prev):
                    assert torch.equal(now[o:o + n], was[o:o + n]), what
    if skip:                                            # c's own bias-correction count: 3 of the 5 steps
        assert int(ropt.state[ref.c]['step']) == 3 and opt._lag == [0, 0, 2, 0] and opt.t == 5
    if mode == "value":
        assert all(x is None for x in norms)


@pytest.mark.parametrize("mode", ["value", "norm"])
@pytest.mark.parametrize("skip", [False, True], ids=["all-reached", "c-skips-2-and-3"])
def test_fused_adamw_groups_against_torch_adamw(mode, skip):
    from frankenstein_amd.utils import train_utils as tu
    _check_four_against_torch(tu, mode, skip)


@pytest.mark.parametrize("mode", ["value", "norm"])
def test_fused_adamw_groups_resume_from_state_dict(mode):
    """state_dict() after step 3 into a fresh optimizer built with other defaults: steps 4 and 5 repeat the uninterrupted run's bits
    (step count, lags, moments and every group's lr / lr_scale / decay / betas travel)"""
    from frankenstein_amd.utils import train_utils as tu
    whole, _, _ = _run_four(tu, mode, True)
    resumed, _, opt = _run_four(tu, mode, True, resume_at=3)
    for step in (3, 4):
        for a, b, what in zip(resumed[step], whole[step], ("p", "m", "v")):
            assert torch.equal(a, b), (step, what)
    assert [g['weight_decay'] for g in opt.param_groups] == [0.1, 0.0, 1e-2] and opt.param_groups[1]['lr_scale'] == 0.1


def test_grouped_step_is_one_launch_and_uploads_its_table_once(K, monkeypatch):
    """an unclipped grouped step is ONE kernel launch, a norm-clipped one two; the device table is built on the first step only"""
    from frankenstein_amd.utils import train_utils as tu
    for kw, want in ((dict(grad_clip=1.0), ["fk_adamw_step_groups"]), (dict(grad_clip_norm=1.0), ["fk_grad_sumsq", "fk_adamw_step_groups"])):
        m = _Four().cuda()
        opt = tu.FusedAdamW(m, lr=1e-3, param_groups=_four_groups(m), **kw)
        _four_step(opt, 0, [True] * 4)
        calls, uploads = [], []
        real_call, real_seg = K.call, K.adamw_segments
        monkeypatch.setattr(K, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
        monkeypatch.setattr(K, "adamw_segments", lambda *a: (uploads.append(1), real_seg(*a))[1])
        for step in (1, 2):
            _four_step(opt, step, [True] * 4)
        monkeypatch.undo()
        assert [c for c in calls if "adamw" in c or "sumsq" in c] == want * 2 and not uploads


class _Twenty(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(13)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(5 + 3 * i, generator=g)) for i in range(20)])


@pytest.mark.parametrize("mode", ["value", "norm"])
def test_more_than_16_slots_take_several_launches(K, mode, monkeypatch):
    """20 parameters in two groups that have each sat out another number of steps: 20 (group, step) pairs, so the update is two launches
    over disjoint parts of the table (16 + 4 slots) and, with the norm clip, one norm pass over their union; every parameter against
    float64 with its own bias-correction step"""
    from frankenstein_amd.utils import train_utils as tu
    m = _Twenty().cuda()
    ps = list(m.ps)
    kw = dict(grad_clip=1.0) if mode == "value" else dict(grad_clip_norm=3.0)
    opt = tu.FusedAdamW(m, lr=1e-3, weight_decay=0.1, param_groups=[{'params': ps[1::2], 'weight_decay': 0.0, 'betas': (0.8, 0.95)}], **kw)
    a = opt.arena
    opt.t, opt._lag = 30, list(range(20))                # as if parameter i had missed i of the first 30 steps
    opt.m.copy_(rnd(a.numel, 31, 0.1))
    opt.v.copy_(rnd(a.numel, 32, 0.1).abs())
    a.grad.copy_(rnd(a.numel, 33))
    p0, g0, m0, v0 = (t.detach().cpu().clone() for t in (a.flat, a.grad, opt.m, opt.v))
    opt.mark_touched()
    calls, real_call = [], K.call
    monkeypatch.setattr(K, "call", lambda name, *args: (calls.append(name), real_call(name, *args))[1])
    opt.step()
    monkeypatch.undo()
    want = ["fk_adamw_step_groups"] * 2 if mode == "value" else ["fk_grad_sumsq"] + ["fk_adamw_step_groups"] * 2
    assert [c for c in calls if "adamw" in c or "sumsq" in c] == want
    coef = 1.0
    if mode == "norm":
        cov = torch.cat([g0[o:o + (p.numel() + 3) // 4 * 4] for p, o in zip(a.params, a.offsets)]).double()    # the padding holds gradient too
        total = float(cov.norm())
        np.testing.assert_allclose(float(opt.last_grad_norm), total, rtol=RTOL)
        assert total > 3.0
        coef = 3.0 / (total + 1e-6)
    pd, md, vd = (t.detach().cpu() for t in (a.flat, opt.m, opt.v))
    for i, (p, o) in enumerate(zip(a.params, a.offsets)):
        pg = opt.param_groups[opt._group_of[i]]
        assert opt._group_of[i] == (0 if i % 2 else 1)
        hyper = (pg['lr'], pg['betas'][0], pg['betas'][1], pg['eps'], pg['weight_decay'], 31 - i)
        pr, mr, vr = ref_update(p0, g0, m0, v0, (o, o + p.numel(), 0), hyper, clip=1.0 if mode == "value" else 0.0, coef=coef)
        for got, ref, atol in ((pd, pr, ATOL_PM), (md, mr, ATOL_PM), (vd, vr, ATOL_V)):
            torch.testing.assert_close(got[o:o + p.numel()], ref.float(), rtol=RTOL, atol=atol, msg=lambda t: f"parameter {i}: {t}")
    assert int(torch.count_nonzero(a.grad)) == 0 and opt._lag == list(range(20)) and opt.t == 31


# =============================================================================================== 7: GPT.configure_optimizers
class _AsTrainStepModel(torch.nn.Module):
    """GPT behind the (inputs, labels, date_info) call of train_step / GraphedTrainStep"""

    def __init__(self, gpt):
        super().__init__()
        self.gpt = gpt

    def forward(self, inputs, labels, date_info=None):
        return self.gpt(inputs, targets=labels)


def _gpt_on_gpu():
    from tests.test_models_gpu import load_synth, mk_gpt
    cfgo, _, tk, idx = C.gpt_small(True)
    return load_synth(mk_gpt(cfgo)).cuda(), idx.cuda(), tk.cuda()


def test_gpt_configure_optimizers_returns_the_grouped_arena_optimizer():
    import frankenstein_amd as fa
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype("fp32")
    g, idx, tk = _gpt_on_gpu()
    named = {n: p for n, p in g.named_parameters() if p.requires_grad}               # the reference's rule, models/gpt2_model.py:288-298
    ref_decay, ref_nodecay = [p for p in named.values() if p.dim() >= 2], [p for p in named.values() if p.dim() < 2]
    opt = g.configure_optimizers(0.1, 1e-3, (0.9, 0.95), 'cuda')
    assert type(opt) is tu.FusedAdamW and len(opt.param_groups) == 2
    assert [id(p) for p in opt.param_groups[0]['params']] == [id(p) for p in ref_decay]
    assert [id(p) for p in opt.param_groups[1]['params']] == [id(p) for p in ref_nodecay]
    assert [pg['weight_decay'] for pg in opt.param_groups] == [0.1, 0.0] and all(tuple(pg['betas']) == (0.9, 0.95) for pg in opt.param_groups)
    assert sum(p is g.lm_head.weight for pg in opt.param_groups for p in pg['params']) == 1 and g.transformer.wte.weight is g.lm_head.weight
    assert [p is q for p, q in zip(opt.arena.params, tu._unique_trainable(g))] == [True] * len(opt.arena.params)       # arena order untouched
    opt.param_groups[1]['lr_scale'] = 0.5
    a = opt.arena
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=True, warmup_iters=4, lr_decay_iters=20, learning_rate=1e-3, grad_clip=0.0)
    get_lr = tu.init_lr_scheduler(cfg)
    for step in (1, 2):                                  # train_step's body by hand, so that the gradient can be kept
        _set_lr(opt, get_lr(step))
        assert opt.param_groups[0]['lr'] == get_lr(step) and opt.param_groups[1]['lr'] == get_lr(step) * 0.5
        loss, _ = g(idx, targets=tk)
        loss.backward()
        torch.cuda.synchronize()
        p0, g0, m0, v0 = (t.detach().cpu().clone() for t in (a.flat, a.grad, opt.m, opt.v))
        assert all(opt._touched) and float(g0.abs().max()) > 0
        opt.step()
        assert int(torch.count_nonzero(a.grad)) == 0
        pd, md, vd = (t.detach().cpu() for t in (a.flat, opt.m, opt.v))
        for i, (p, o) in enumerate(zip(a.params, a.offsets)):
            pg = opt.param_groups[opt._group_of[i]]
            assert opt._group_of[i] == (0 if p.dim() >= 2 else 1)
            seg = (o, o + p.numel(), 0)
            pr, mr, vr = ref_update(p0, g0, m0, v0, seg, (pg['lr'], 0.9, 0.95, pg['eps'], pg['weight_decay'], step))
            for got, want, atol in ((pd, pr, ATOL_PM), (md, mr, ATOL_PM), (vd, vr, ATOL_V)):
                torch.testing.assert_close(got[o:o + p.numel()], want.float(), rtol=RTOL, atol=atol, msg=lambda t: f"step {step} parameter {i}: {t}")
    assert len(opt._seg_dev) == 1 and len(next(iter(opt._seg_dev))) > 10          # one table, the groups alternate tensor by tensor


def test_graphed_train_step_with_groups_equals_the_eager_step():
    import frankenstein_amd as fa
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype("bf16")
    cfg = tu.TrainConfig(mixed_precision=True, use_scheduler=True, warmup_iters=2, lr_decay_iters=10, learning_rate=1e-3, grad_clip=0.0)
    runs = []
    for graphed in (False, True):
        g, idx, tk = _gpt_on_gpu()
        opt = g.configure_optimizers(0.1, 1e-3, (0.9, 0.95), 'cuda')
        opt.param_groups[1]['lr_scale'] = 0.5
        model = _AsTrainStepModel(g)
        batch = (idx, tk, None)
        if graphed:
            step = tu.GraphedTrainStep(model, batch, opt, cfg)
            losses = [float(step(batch, i)) for i in range(1, 4)]
        else:
            losses = [float(tu.train_step(model, batch, opt, i, cfg)) for i in range(1, 4)]
        assert opt.t == 3 and opt.param_groups[1]['lr'] == tu.init_lr_scheduler(cfg)(3) * 0.5
        runs.append((losses, opt.arena.flat.detach().clone(), opt.m.clone(), opt.v.clone()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b, what in zip(runs[0][1:], runs[1][1:], ("p", "m", "v")):
        assert torch.equal(a, b), what
    assert runs[0][0][-1] < runs[0][0][0]


# =============================================================================================== 8: data parallel
DP_CLIP = 1e-2            # far below the gradient norm of the first steps: every step is clipped


def _dp_optimizer(tu, m, **kw):
    groups = tu.decay_groups(m, 0.1)
    groups[1]['lr_scale'] = 0.5
    return tu.FusedAdamW(m, lr=1e-3, param_groups=groups, grad_clip_norm=DP_CLIP, **kw)


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from tests.test_dp_gpu import _batch, _build
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from frankenstein_amd.utils import train_utils as tu
    m = _build()
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3, grad_clip=0.0)
    opt = _dp_optimizer(tu, m, bucket_bytes=64 << 10)
    assert opt.sync.world == world and len(opt.sync.buckets) > 1
    x, y = _batch(4)
    norms = []
    for step in range(3):
        xb, yb, _ = tu.shard_batch((x, y, None), rank, world)
        tu.train_step(m, (xb, yb, None), opt, step, cfg)
        norms.append(float(opt.last_grad_norm))
    torch.cuda.synchronize()
    out[rank] = (opt.arena.flat.detach().cpu().numpy(), norms)
    dist.destroy_process_group()


def test_two_ranks_with_groups_and_norm_clip_stay_identical_and_equal_one_rank():
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _batch, _build, _free_port
    world = 2
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert len(out) == world
    np.testing.assert_array_equal(out[0][0], out[1][0])          # the same norm bits on both ranks -> the same coefficient -> the same bits
    assert out[0][1] == out[1][1] and min(out[0][1]) > DP_CLIP
    from frankenstein_amd.utils import train_utils as tu
    m = _build()
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3, grad_clip=0.0)
    opt = _dp_optimizer(tu, m)
    x, y = _batch(4)
    for step in range(3):
        tu.train_step(m, (x, y, None), opt, step, cfg)
    ref = opt.arena.flat.detach().cpu().numpy()
    diff = np.abs(out[0][0] - ref)                       # the bound of tests/test_dp_gpu.py
    assert np.quantile(diff, 0.99) < 2e-5 and diff.max() < 5e-3, (np.quantile(diff, 0.99), diff.max())
