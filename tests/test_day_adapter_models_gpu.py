"""The per-session input adapter through the models (tiny config: window 32, 16 electrodes, patch 4):
  * n_days = 0: date_info changes nothing, bit for bit;
  * n_days = 3 with the zero adapter: BrainFormer, BrainFormerCE, BrainFormerCTC, Franky and MAE (fixed indices) give the loss and outputs
    of the n_days = 0 model with the same other weights, torch.equal, for any date_info;
  * a random adapter, fp32 mode: outputs equal those of the n_days = 0 model fed with x' = x + x @ delta[d] + bias[d] computed on the
    host in float64 and cast to fp32, within the project's fp32 bound of 1e-3 on logits, and the gradients of all shared parameters agree
    within check_full_grads' bounds of tests/test_models_gpu.py (rtol 1e-3, atol 2e-5);
  * three train_steps with FusedAdamW (param_groups with an lr_scale for the adapter): the slices of the days present move, those of
    absent days stay exactly zero; GraphedTrainStep gives the eager parameters with another date_info in every replay;
  * data parallel (the pattern of tests/test_dp_gpu.py): the ranks see different days and end with identical delta and bias;
  * inference: BrainFormerCTC.decode / align / error_rate and Franky.generate_beam / generate / rescore with date_info equal the calls
    on the host-adapted x' without an adapter, ids identical."""
import os

import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import synth
from tests import day_adapter_ref as DR
from tests.test_dp_gpu import _free_port

pytestmark = pytest.mark.gpu

B, T, C, P, ND = 4, 32, 16, 4, 3
DAYS = [2, 0, -1, 2]                          # day 1 is absent, sample 2 has no session


@pytest.fixture(autouse=True)
def _fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def configs(n_days):
    from frankenstein_amd.models import brainformer as bf
    enc = bf.MAEConfig(window_size=T, n_electrodes=C, patch_size=P, dim=64, n_layers=2, head_dim=16, hidden_dim=128, n_heads=4, n_kv_heads=4,
                       n_dec_layers=2, decoder_dim=64, n_days=n_days)
    return enc, bf.Config(encoder=enc, n_output_tokens=8, output_dim=12, dim=64, n_layers=1, head_dim=16, hidden_dim=96, n_heads=4, n_kv_heads=4)


def adapter_of(m):
    return next(mod for mod in m.modules() if type(mod).__name__ == "DayAdapter")


def load(m, adapter=None):
    """synthetic weights by key name (the same for every n_days); the adapter zero, or (delta, bias)"""
    sd = m.state_dict()
    st = synth.make_state({k: tuple(v.shape) for k, v in sd.items() if v is not None and "day_adapter" not in k})
    for k in list(st):
        if k.endswith("lm_head.weight"):
            st[k] = st[k.replace("lm_head.weight", "transformer.wte.weight")]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    m = m.cuda()
    if adapter is not None:
        ad = adapter_of(m)
        with torch.no_grad():
            ad.delta.copy_(torch.from_numpy(adapter[0]))
            ad.bias.copy_(torch.from_numpy(adapter[1]))
    return m


def make(kind, n_days, adapter=None):
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models import gpt2_model as g2
    from frankenstein_amd.models import notebook_models as nm
    enc, cfg = configs(n_days)
    if kind == "mae":
        return load(bf.MAE(enc), adapter)
    if kind == "franky":
        enc, cfg = configs(n_days)
        cfg.output_dim = 32
        gpt = g2.GPT(g2.GPTConfig(block_size=64, vocab_size=50257, n_layer=1, n_head=2, n_embd=32, dropout=0.0, bias=True))
        return load(nm.Franky(nm.BrainEncoder(cfg), gpt), adapter)
    return load({"bf": bf.BrainFormer, "ce": nm.BrainFormerCE, "ctc": nm.BrainFormerCTC}[kind](cfg), adapter)


def batch(kind):
    x = torch.from_numpy(synth.make_inputs(B, T, C)).cuda()
    if kind == "bf":
        return x, torch.from_numpy(synth.make_motion_targets(B, 8, 12)).cuda(), {}
    if kind == "ce":
        return x, torch.from_numpy(np.random.default_rng(1).integers(0, 12, (B, 8))).cuda(), {}
    if kind == "ctc":
        t = np.random.default_rng(2).integers(0, 11, (B, 3))
        t[1, 2:] = -100
        return x, torch.from_numpy(t).cuda(), {}
    if kind == "franky":
        return x, torch.from_numpy(synth.make_tokens(B, 12)).cuda(), {}
    masked = torch.stack([torch.sort(torch.randperm(128, generator=torch.Generator().manual_seed(b))[:96])[0] for b in range(B)])
    rest = torch.stack([torch.tensor(sorted(set(range(128)) - set(r.tolist()))) for r in masked])
    return x, None, dict(indices=(masked.cuda(), rest.cuda()), masking_ratio=0.75, return_preds=True)


def random_adapter(seed=11, scale=1.0):
    rng = np.random.default_rng(seed)
    delta = (scale * rng.standard_normal((ND, C, C)) / np.sqrt(C)).astype(np.float32)
    bias = (scale * (rng.standard_normal((ND, C)) + np.arange(ND)[:, None])).astype(np.float32)
    return delta, bias


def host_adapted(x, days, adapter):
    """x' in float64 on the host, cast to fp32"""
    return torch.from_numpy(DR.adapt(x.cpu().numpy(), None if days is None else np.asarray(days), *adapter).astype(np.float32)).cuda()


def outputs(m, x, y, kw, date_info=None):
    out = m(x, y, date_info=date_info, **kw)
    return [o for o in out if o is not None]


def test_no_adapter_ignores_date_info():
    m = make("bf", 0)
    x, y, kw = batch("bf")
    a = outputs(m, x, y, kw)
    for di in (torch.tensor(DAYS), 1, torch.tensor(DAYS, dtype=torch.int32).cuda()):
        b = outputs(m, x, y, kw, di)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert not hasattr(m.encoder, "day_adapter") and not m.encoder.day_active(torch.tensor(DAYS))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["bf", "ce", "ctc", "franky", "mae"])
def test_zero_adapter_equals_no_adapter(kind, mode):
    fa.set_compute_dtype(mode)
    x, y, kw = batch(kind)
    want = outputs(make(kind, 0), x, y, kw)
    m = make(kind, ND)
    assert len(want) >= 2 or kind == "mae"
    for di in (torch.tensor(DAYS).cuda(), torch.tensor(DAYS, dtype=torch.int32), 7, 1, None):
        got = outputs(m, x, y, kw, di)
        assert len(got) == len(want)
        for p, q in zip(got, want):
            assert torch.equal(p, q), (kind, di)
    with torch.no_grad():                      # inference with date_info=None: the path without the adapter, same bits again
        assert not m.brain_model.encoder.day_active(None) if kind == "franky" else not m.encoder.day_active(None)
        for p, q in zip(outputs(m, x, y, kw), want):
            assert torch.equal(p, q)


@pytest.mark.parametrize("kind", ["bf", "ce"])
def test_random_adapter_equals_host_adapted_input(kind):
    adapter = random_adapter()
    x, y, kw = batch(kind)
    m, m0 = make(kind, ND, adapter), make(kind, 0)
    xp = host_adapted(x, DAYS, adapter)
    assert float((xp - x).abs().max()) > 1.0
    for di in (torch.tensor(DAYS), 2):
        loss, out = m(x, y, date_info=di)
        loss0, out0 = m0(host_adapted(x, DAYS if torch.is_tensor(di) else [di] * B, adapter), y)
        err = float((out.float() - out0.float()).abs().max())
        print(f"MODEL {kind} logits max |adapter route - host route| {err:.3e}")
        assert err < 1e-3 and abs(float(loss) - float(loss0)) < 1e-4
    loss.backward()
    loss0.backward()
    g0 = dict(m0.named_parameters())
    n = 0
    for k, p in m.named_parameters():
        if "day_adapter" in k:
            continue
        np.testing.assert_allclose(p.grad.cpu().numpy(), g0[k].grad.cpu().numpy(), rtol=1e-3, atol=2e-5, err_msg=k)
        n += 1
    assert n == len(g0)
    ad = adapter_of(m)
    assert float(ad.delta.grad[2].abs().max()) > 0 and float(ad.delta.grad[0].abs().max()) == 0.0 and float(ad.delta.grad[1].abs().max()) == 0.0


def test_mae_adapts_the_encoder_input_only():
    """the adapter changes the encoder's tokens; the reconstruction target stays the raw patches"""
    adapter = random_adapter()
    x, y, kw = batch("mae")
    m, m0 = make("mae", ND, adapter), make("mae", 0)
    loss, rec, bm = m(x, date_info=torch.tensor(DAYS), **kw)
    loss0, rec0, bm0 = m0(x, **kw)
    vis = bm == 0                              # kept patches are returned as they came in: raw
    assert torch.equal(rec[vis], rec0[vis]) and torch.equal(bm, bm0)
    assert not torch.equal(rec[0], rec0[0]) and torch.equal(rec[2], rec0[2])       # sample 2 has no session: untouched
    loss.backward()
    ad = adapter_of(m)
    assert float(ad.delta.grad[2].abs().max()) > 0 and float(ad.delta.grad[1].abs().max()) == 0.0 and float(ad.bias.grad[0].abs().max()) > 0


def _opt(m, tu, cfg, **kw):
    ad = adapter_of(m)
    return tu.FusedAdamW(m, lr=1e-3, weight_decay=cfg.weight_decay, grad_clip=cfg.grad_clip,
                         param_groups=[dict(params=[ad.delta, ad.bias], lr_scale=2.0, weight_decay=0.05)], **kw)


STEP_DAYS = ([2, 0, -1, 2], [0, 0, 0, 0], [2, 2, 3, -1])         # day 1 never occurs


def test_train_steps_and_graphed_step():
    from frankenstein_amd.utils import train_utils as tu
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3)
    x, y, _ = batch("bf")
    m = make("bf", ND)
    opt = _opt(m, tu, cfg)
    ad = adapter_of(m)
    assert getattr(ad.delta, "_fk_arena", False) and getattr(ad.bias, "_fk_arena", False)          # ordinary parameters of the arena
    for step, days in enumerate(STEP_DAYS):
        tu.train_step(m, (x, y, torch.tensor(days)), opt, step, cfg)
    for d in (0, 2):
        assert float(ad.delta[d].abs().max()) > 0 and float(ad.bias[d].abs().max()) > 0
    assert float(ad.delta[1].abs().max()) == 0.0 and float(ad.bias[1].abs().max()) == 0.0
    eager = opt.arena.flat.detach().clone()
    # the same three steps as one captured graph, date_info copied into the static batch (int32 on the host in one call)
    m2 = make("bf", ND)
    opt2 = _opt(m2, tu, cfg)
    gs = tu.GraphedTrainStep(m2, (x, y, torch.tensor(STEP_DAYS[0]).cuda()), opt2, cfg, warmup=1)
    for step, days in enumerate(STEP_DAYS):
        gs((x, y, torch.tensor(days, dtype=torch.int32 if step == 1 else torch.int64)), step)
    torch.cuda.synchronize()
    assert torch.equal(opt2.arena.flat.detach(), eager)


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from frankenstein_amd.utils import train_utils as tu
    fa.set_compute_dtype("fp32")
    m = make("bf", ND)
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3)
    opt = tu.FusedAdamW(m, lr=1e-3, weight_decay=cfg.weight_decay, grad_clip=cfg.grad_clip, bucket_bytes=64 << 10)
    x, y, _ = batch("bf")
    days = torch.tensor([0, 0, 2, 2])                               # rank 0 sees day 0 only, rank 1 day 2 only
    for step in range(2):
        tu.train_step(m, tu.shard_batch((x, y, days), rank, world), opt, step, cfg)
    torch.cuda.synchronize()
    ad = adapter_of(m)
    out[rank] = (ad.delta.detach().cpu().numpy(), ad.bias.detach().cpu().numpy())
    dist.destroy_process_group()


def test_data_parallel_ranks_see_different_days():
    import torch.multiprocessing as mp
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    (d0, b0), (d1, b1) = out[0], out[1]
    np.testing.assert_array_equal(d0, d1)
    np.testing.assert_array_equal(b0, b1)
    for d in (0, 2):                          # each rank's day moved on BOTH ranks
        assert np.abs(d0[d]).max() > 0 and np.abs(b0[d]).max() > 0
    assert np.abs(d0[1]).max() == 0.0 and np.abs(b0[1]).max() == 0.0


def test_inference_entry_points():
    adapter = random_adapter(scale=0.5)
    x, y, _ = batch("ctc")
    di = torch.tensor(DAYS)
    xp = host_adapted(x, DAYS, adapter)
    ctc, ctc0 = make("ctc", ND, adapter).eval(), make("ctc", 0).eval()
    for kw in ({}, dict(beam_width=4), dict(beam_width=4, nbest=2)):
        got, want = ctc.decode(x, date_info=di, **kw), ctc0.decode(xp, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), kw
    assert not torch.equal(ctc.features(x, di), ctc.features(x))
    a, a0 = ctc.align(x, y, date_info=di), ctc0.align(xp, y)
    assert torch.equal(a.path, a0.path)
    e, e0 = ctc.error_rate(x, y, date_info=di), ctc0.error_rate(xp, y)
    assert torch.equal(e[1], e0[1])
    fr, fr0 = make("franky", ND, adapter).eval(), make("franky", 0).eval()
    xn, xpn = x.cpu().numpy(), xp.cpu().numpy()
    torch.manual_seed(5)
    got = fr.generate_beam(xn, max_new_tokens=5, beam_width=3, date_info=di)
    torch.manual_seed(5)
    want = fr0.generate_beam(xpn, max_new_tokens=5, beam_width=3)
    assert got.shape == (B, 6) and torch.equal(got, want)
    torch.manual_seed(5)
    one = fr.generate_beam(xn[0], max_new_tokens=5, beam_width=3, date_info=DAYS[0])
    torch.manual_seed(5)
    assert torch.equal(one, fr0.generate_beam(xpn[0], max_new_tokens=5, beam_width=3))
    torch.manual_seed(6)
    got = fr.generate(xn[1], max_new_tokens=4, top_k=1, date_info=DAYS[1])
    torch.manual_seed(6)
    assert torch.equal(got, fr0.generate(xpn[1], max_new_tokens=4, top_k=1))
    ids, lengths, scores = ctc0.decode(xp, beam_width=4, nbest=2)
    ids = ids.clamp(min=-100)
    r, r0 = fr.rescore(x, ids, lengths, scores, date_info=di), fr0.rescore(xp, ids, lengths, scores)
    assert torch.equal(r[0], r0[0])
