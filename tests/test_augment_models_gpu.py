"""The signal augmentation through the models (tiny config: window 32, 16 electrodes, patch 4):
  * train(): an Encoder with augmentation equals, bit for bit, a copy without it fed engine.augment_signal(x) drawn at the same step
    word (both compute modes): the fused tokeniser draws exactly the stand-alone signal;
  * eval(): the un-augmented model bit for bit, and the step word is left alone;
  * with n_days > 0 the outputs and the gradients of delta and bias equal those of the model without augmentation on the augmented signal;
  * MAE / SimpleMAE: the target, the padding mask and the kept patches come from the clean x, only the encoder's input changes;
  * train_step with augmentation runs and changes the loss, two consecutive steps draw different noise, and GraphedTrainStep ends
    with the eager parameters: every replay draws the next step's noise."""
import numpy as np
import pytest
import torch

import frankenstein_amd as fa
from frankenstein_amd import engine as E
from frankenstein_amd import kernels as K
from frankenstein_amd import synth

pytestmark = pytest.mark.gpu

B, T, C, P, ND = 4, 32, 16, 4, 3
DAYS = [2, 0, -1, 2]
AUG = dict(aug_white_sd=0.5, aug_offset_sd=0.2, aug_chan_drop=0.1, aug_time_masks=2, aug_time_mask_len=6)
AUG_SHIFT = dict(AUG, aug_time_shift=3)


@pytest.fixture(autouse=True)
def _fp32_mode():
    fa.set_compute_dtype("fp32")
    yield
    fa.set_compute_dtype("bf16")


def configs(n_days=0, **aug):
    from frankenstein_amd.models import brainformer as bf
    enc = bf.MAEConfig(window_size=T, n_electrodes=C, patch_size=P, dim=64, n_layers=2, head_dim=16, hidden_dim=128, n_heads=4, n_kv_heads=4,
                       n_dec_layers=2, decoder_dim=64, n_days=n_days, **aug)
    return enc, bf.Config(encoder=enc, n_output_tokens=8, output_dim=12, dim=64, n_layers=1, head_dim=16, hidden_dim=96, n_heads=4, n_kv_heads=4)


def load(m, adapter=False):
    """synthetic weights by key name: the same for a model with and without augmentation (it adds no key)"""
    sd = m.state_dict()
    st = synth.make_state({k: tuple(v.shape) for k, v in sd.items() if v is not None and "day_adapter" not in k})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    m = m.cuda()
    if adapter:
        rng = np.random.default_rng(11)
        with torch.no_grad():
            m.encoder.day_adapter.delta.copy_(torch.from_numpy((rng.standard_normal((ND, C, C)) / np.sqrt(C)).astype(np.float32)))
            m.encoder.day_adapter.bias.copy_(torch.from_numpy(rng.standard_normal((ND, C)).astype(np.float32)))
    return m


def make(kind, n_days=0, **aug):
    from frankenstein_amd.models import brainformer as bf
    enc, cfg = configs(n_days, **aug)
    if kind == "enc":
        return load(bf.Encoder(enc))
    if kind == "mae":
        return load(bf.MAE(enc))
    return load(bf.BrainFormer(cfg), adapter=n_days > 0)


def inputs():
    return torch.from_numpy(synth.make_inputs(B, T, C)).cuda()


def step_word(dev):
    torch.cuda.synchronize()
    return int(E.augment_words(dev)[1])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training_encoder_equals_plain_encoder_on_the_augmented_signal(mode):
    fa.set_compute_dtype(mode)
    x = inputs()
    m, m0 = make("enc", **AUG_SHIFT).train(), make("enc").train()
    s = step_word(x.device)
    out = m(x)
    assert step_word(x.device) == s + 1                            # one forward: one step
    xa = E.augment_signal(x, m.augment)                            # drawn at the word the forward used
    assert step_word(x.device) == s + 1 and not torch.equal(xa, x)
    assert torch.equal(out, m0(xa))
    assert not torch.equal(out, m0(x))
    out2 = m(x)                                                    # the next forward: the next step's noise
    assert step_word(x.device) == s + 2 and not torch.equal(out2, out)
    assert torch.equal(out2, m0(E.augment_signal(x, m.augment)))


def test_eval_is_the_plain_model_and_leaves_the_step_word_alone():
    x = inputs()
    y = torch.from_numpy(synth.make_motion_targets(B, 8, 12)).cuda()
    m, m0 = make("bf", **AUG_SHIFT).eval(), make("bf").eval()
    s = step_word(x.device)
    with torch.no_grad():
        a, b = m(x, y), m0(x, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and step_word(x.device) == s
    m.train(), m0.train()
    assert not torch.equal(m(x, y)[1], m0(x, y)[1]) and step_word(x.device) == s + 1
    off = make("bf").train()                                       # all knobs zero in train(): today's forward, nothing advanced
    assert torch.equal(off(x, y)[1], m0(x, y)[1]) and step_word(x.device) == s + 1


def test_day_adapter_sees_the_augmented_signal():
    x = inputs()
    y = torch.from_numpy(synth.make_motion_targets(B, 8, 12)).cuda()
    di = torch.tensor(DAYS)
    m, m0 = make("bf", ND, **AUG_SHIFT).train(), make("bf", ND).train()
    loss, out = m(x, y, date_info=di)
    xa = E.augment_signal(x, m.encoder.augment)
    loss0, out0 = m0(xa, y, date_info=di)
    assert torch.equal(out, out0) and torch.equal(loss, loss0)
    loss.backward()
    loss0.backward()
    ad, ad0 = m.encoder.day_adapter, m0.encoder.day_adapter
    assert torch.equal(ad.delta.grad, ad0.delta.grad) and torch.equal(ad.bias.grad, ad0.bias.grad)
    assert float(ad.delta.grad[2].abs().max()) > 0 and float(ad.delta.grad[1].abs().max()) == 0.0
    plain = make("bf", ND).train()                                 # and they are not the gradients of the clean signal
    plain(x, y, date_info=di)[0].backward()
    assert not torch.equal(plain.encoder.day_adapter.delta.grad, ad.delta.grad)


def _mae_batch():
    masked = torch.stack([torch.sort(torch.randperm(128, generator=torch.Generator().manual_seed(b))[:96])[0] for b in range(B)])
    rest = torch.stack([torch.tensor(sorted(set(range(128)) - set(r.tolist()))) for r in masked])
    return dict(indices=(masked.cuda(), rest.cuda()), masking_ratio=0.75, return_preds=True)


def test_mae_augments_the_encoder_input_only():
    x, kw = inputs(), _mae_batch()
    m, m0 = make("mae", **AUG).train(), make("mae").train()
    seen = []
    orig = E.MaskedPatchEmbed.apply
    try:                                                           # what reaches the encoder's embedding
        E.MaskedPatchEmbed.apply = staticmethod(lambda tok_all, *a: (seen.append(tok_all), orig(tok_all, *a))[1])
        loss, rec, bm = m(x, **kw)
    finally:
        del E.MaskedPatchEmbed.apply                              # back to the inherited Function.apply
    loss0, rec0, bm0 = m0(x, **kw)
    xa = E.augment_signal(x, m.encoder.augment)
    assert torch.equal(seen[0].view(-1, 32), K.patchify(xa, P, 32, torch.float32))          # the encoder saw the augmented patches
    vis = bm == 0
    assert torch.equal(bm, bm0) and torch.equal(rec[vis], rec0[vis]) and torch.equal(rec0[vis], x[vis])   # kept patches: the clean x
    assert not torch.equal(rec[~vis], rec0[~vis]) and float(loss.detach()) != float(loss0.detach())
    # the target is the clean x: the loss is the MSE of the predictions against the clean masked patches
    want = torch.mean((rec[~vis] - x[~vis]) ** 2)
    assert abs(float(loss.detach()) - float(want)) <= 1e-5 * max(1.0, float(want))
    m.eval()
    with torch.no_grad():
        l1 = m(x, **kw)[0]
        l0 = m0.eval()(x, **kw)[0]
    assert torch.equal(l1, l0)


def test_simple_mae_keeps_padding_and_clean_targets():
    from frankenstein_amd.models import simple_mae as sm
    Ts, Cs = 16, 8
    aug = dict(aug_white_sd=0.5, aug_offset_sd=0.2, aug_chan_drop=0.2, aug_time_masks=1, aug_time_mask_len=4)
    mk = lambda **a: (sm.SimpleEncoderConfig(block_size=Ts, patch_size=Cs, n_layers=1, dim=32, hidden_dim=64, head_dim=16, n_heads=2, n_kv_heads=2, **a),
                      sm.SimpleMAEConfig(n_layers=1, dim=32, hidden_dim=64, head_dim=16, n_heads=2, n_kv_heads=2))
    m, m0 = load(sm.SimpleMAE(*mk(**aug))).train(), load(sm.SimpleMAE(*mk())).train()
    x = torch.from_numpy(synth.make_inputs(B, Ts, Cs)).cuda()
    x[:, 12:] = 0.0                                                # a padded tail
    masked = torch.stack([torch.sort(torch.randperm(Ts, generator=torch.Generator().manual_seed(b))[:12])[0] for b in range(B)])
    rest = torch.stack([torch.tensor(sorted(set(range(Ts)) - set(r.tolist()))) for r in masked])
    kw = dict(indices=(masked.cuda(), rest.cuda()), return_preds=True)
    seen = []
    h = m.encoder.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    s = step_word(x.device)
    loss, rec, bm = m(x, **kw)
    h.remove()
    assert step_word(x.device) == s + 1                            # SimpleMAE augments once; its encoder does not augment again
    loss0, rec0, bm0 = m0(x, **kw)
    xa = E.augment_signal(x, m.encoder.augment)
    assert torch.equal(xa[:, 12:], torch.zeros_like(xa[:, 12:])) and not torch.equal(xa[:, :12], x[:, :12])     # padding stays padding
    assert torch.equal(seen[0], K.gather_rows(xa, rest.cuda()))
    vis = bm == 0
    assert torch.equal(bm, bm0) and torch.equal(rec[vis], rec0[vis]) and float(loss.detach()) != float(loss0.detach()) and np.isfinite(float(loss.detach()))
    # the stand-alone encoder augments its own input in train(), and only there
    enc = m.encoder
    out = enc(x)
    assert step_word(x.device) == s + 2 and torch.equal(out, m0.encoder(E.augment_signal(x, enc.augment)))
    assert torch.equal(enc.eval()(x), m0.encoder.eval()(x)) and step_word(x.device) == s + 2


def test_signal_augment_module():
    from frankenstein_amd.models.brainformer import SignalAugment
    x = inputs()
    cfg = E.AugmentConfig(white_sd=0.3, time_shift=2)
    mod = SignalAugment(cfg).cuda()
    s = step_word(x.device)
    y = mod(x)
    assert step_word(x.device) == s + 1 and y.shape == x.shape and y.dtype == torch.float32
    assert torch.equal(y, E.augment_signal(x, cfg)) and not torch.equal(y, x)
    assert mod.eval()(x) is x and step_word(x.device) == s + 1


def test_train_steps_and_graphed_step():
    from frankenstein_amd.utils import train_utils as tu
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3)
    x = inputs()
    y = torch.from_numpy(synth.make_motion_targets(B, 8, 12)).cuda()
    words = E.augment_words(x.device)
    m, m0 = make("bf", **AUG_SHIFT), make("bf")
    opt, opt0 = (tu.FusedAdamW(mm, lr=1e-3, weight_decay=cfg.weight_decay, grad_clip=cfg.grad_clip) for mm in (m, m0))
    words[1] = 100
    losses = [float(tu.train_step(m, (x, y, None), opt, step, cfg)) for step in range(3)]
    assert step_word(x.device) == 103
    l0 = float(tu.train_step(m0, (x, y, None), opt0, 0, cfg))
    assert step_word(x.device) == 103 and np.isfinite(losses).all() and losses[0] != l0
    eager = opt.arena.flat.detach().clone()
    # two forwards on the same weights draw different noise
    m.train()
    a, b = m(x, y)[0].detach(), m(x, y)[0].detach()
    assert float(a) != float(b)
    # the same three steps as one captured graph: every replay draws the next step's noise
    m2 = make("bf", **AUG_SHIFT)
    opt2 = tu.FusedAdamW(m2, lr=1e-3, weight_decay=cfg.weight_decay, grad_clip=cfg.grad_clip)
    gs = tu.GraphedTrainStep(m2, (x, y, None), opt2, cfg, warmup=1)
    words[1] = 100
    got = [float(gs((x, y, None), step)) for step in range(3)]
    assert step_word(x.device) == 103
    assert torch.equal(opt2.arena.flat.detach(), eager) and got == losses
