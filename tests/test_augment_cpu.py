"""Host-side checks of the signal augmentation (csrc/augment.hip, engine.AugmentConfig, models.brainformer.SignalAugment):
  * Philox known answers through the vectorised path of the restatement (tests/augment_ref.py), and the statistics of its draws;
  * each planted defect breaks the bound of tests/test_augment_gpu.py on a named case, on more than 5 % of the elements;
  * argument validation returns FK_EINVAL without a GPU; header, binding and wrappers agree; augment_seed; all-zero config fields leave
    the state-dict key sets unchanged; MAE / SimpleMAE refuse a shift."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import augment_ref as AR
from tests.sample_ref import philox4x32_10

ROOT = Path(__file__).resolve().parents[1]
WORDS = (0x1234567, 5)


def test_philox_known_answers_through_the_vectorised_path():
    # Random123's kat_vectors for philox4x32-10
    kats = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kats:
        assert tuple(philox4x32_10(key, ctr)) == want
        arr = tuple(np.full(3, c, np.uint64) for c in ctr)
        got = philox4x32_10(key, arr)
        assert all(np.all(np.asarray(g) == np.uint64(w)) for g, w in zip(got, want))
    w = AR.blocks(WORDS, np.arange(7)[:, None], np.arange(3)[None, :], 2, AR.WHITE)       # the restatement's call: broadcast counters
    for i in range(7):
        for j in range(3):
            assert [int(v) for v in w[i, j]] == philox4x32_10(WORDS, (i, j, 2, AR.TAG | AR.WHITE))


def test_uniforms_are_exact_in_fp32_and_never_0_or_1():
    w = np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF]], np.uint64)
    for a in (0, 2):
        u1 = ((w[..., a] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        assert np.all(u1.astype(np.float32).astype(np.float64) == u1) and np.all((u1 > 0) & (u1 < 1))
    assert np.float32((float(0xFFFFFFFF >> 8) + 0.5) / 2.0 ** 24) == np.float32(1.0)          # why the rule shifts by 9, not 8
    assert np.all(np.isfinite(AR.normals(w))) and np.all(np.isfinite(AR.normals(w, np.float32)))


def test_white_noise_statistics():
    B, T, C = 2, 32, 256
    n = AR.white_normals(WORDS, B, T, C)
    N = n.size
    assert N == 16384
    se = 1.0 / np.sqrt(N)
    print("white noise: mean %.4f sd %.4f" % (n.mean(), n.std()))
    assert abs(n.mean()) <= 4 * se
    assert abs(n.std() - 1.0) <= 4 * se / np.sqrt(2.0)                  # standard error of the sd of N normals
    z = (n - n.mean()) / n.std()
    lag_t = float(np.mean(z[:, 1:, :] * z[:, :-1, :]))
    lag_c = float(np.mean(z[:, :, 1:] * z[:, :, :-1]))
    print("white noise: lag-1 correlation along time %.4f, along channel %.4f" % (lag_t, lag_c))
    assert abs(lag_t) <= 4 / np.sqrt(z[:, 1:, :].size) and abs(lag_c) <= 4 / np.sqrt(z[:, :, 1:].size)
    n2 = AR.white_normals((WORDS[0], WORDS[1] + 1), B, T, C)            # the next step: another stream
    assert abs(float(np.mean(z * (n2 - n2.mean()) / n2.std()))) <= 4 * se


def test_offset_is_constant_in_time_and_differs_across_samples_and_channels():
    B, T, C = 4, 6, 40
    x = np.zeros((B, T, C), np.float32)
    y = AR.augment(x, AR.Cfg(offset_sd=1.0, keep_padding=False), WORDS)
    assert np.all(y == y[:, :1, :])
    o = AR.offset_normals(WORDS, B, C)
    assert np.array_equal(y[:, 0, :], o) and np.unique(o).size == B * C
    assert abs(o.mean()) <= 4 / np.sqrt(o.size)


def test_drop_and_span_rates():
    B, C, p = 64, 256, 0.3
    d = AR.dropped(WORDS, B, C, p)
    assert abs(d.mean() - p) <= 4 * np.sqrt(p * (1 - p) / d.size)
    assert not AR.dropped(WORDS, B, C, 0.0).any() and AR.dropped(WORDS, B, C, np.nextafter(np.float32(1), np.float32(0))).mean() > 0.999
    # one span of length uniform on 0 .. L, start uniform on 0 .. T - len: the expected share of masked frames is E[len] / T = L / (2 T)
    B, T, L = 4096, 40, 10
    st, ln = AR.spans(WORDS, B, T, 1, L)
    assert ln.min() == 0 and ln.max() == L and st.min() == 0 and np.all(st + ln <= T) and (st + ln).max() == T
    cov = AR.span_mask(WORDS, B, T, 1, L).mean(axis=1)                  # per sample: len / T
    assert np.allclose(cov, ln[:, 0] / T)
    sd_len = np.sqrt(((L + 1) ** 2 - 1) / 12.0)
    assert abs(cov.mean() - L / (2.0 * T)) <= 4 * sd_len / T / np.sqrt(B)
    s = AR.shifts(WORDS, 4096, 3)
    assert s.min() == -3 and s.max() == 3 and abs(s.mean()) <= 4 * 2.0 / np.sqrt(4096)


def test_all_zero_config_is_the_identity_and_rounding_is_one_rounding():
    for c in AC.CASES[:: len(AC.variants(8))]:
        x = c.x()
        assert np.array_equal(AR.augment(x, AR.Cfg(), c.words), x.astype(np.float64))
        ref = AR.forward(x, c.cfg, c.words, c.P, c.ldp)
        assert np.all(ref[:, :, c.P:] == 0.0)
        for dt in c.dtypes:
            r = AR.forward(x, c.cfg, c.words, c.P, c.ldp, dtype=dt)
            assert np.all(np.abs(r - ref) <= AR.half_ulp(ref, dt) * (1 + 1e-9)) and np.array_equal(AR.round_to(r, dt), r)


def test_float32_chain_error_is_of_the_order_of_an_ulp():
    """the yardstick itself: per unit sd the float32 chain is within a few 1e-7 .. 1e-6 of the float64 rule, never 0 with noise on"""
    for cid in ("B2_T50_C256_P25_ld32-white", "B2_T50_C256_P25_ld32-all", "B4_T32_C16_P1_ld1-offset"):
        c = AC.BY_ID[cid]
        _, b = AR.bound(c.x(), c.cfg, c.words, c.P, c.ldp)
        print(cid, "bound", b)
        assert 2e-7 < b < 2e-5


# defect -> the cases it must break
DEFECT_CASES = {
    "noise_by_source_frame": ["B2_T50_C256_P25_ld32-shift_pad", "B4_T32_C16_P1_ld1-all"],
    "offset_varies_in_time": ["B2_T50_C256_P25_ld32-offset", "B2_T12_C6_P3_ld4-offset"],
    "masks_before_noise": ["B2_T50_C256_P25_ld32-mask_full", "B3_T15_C40_P5_ld32-spans8", "B2_T50_C256_P25_ld32-drop_hi"],
    "noise_on_padding": ["B2_T50_C256_P25_ld32-padded", "B2_T12_C6_P3_ld4-shift_pad"],
    "step_ignored": ["B2_T50_C256_P25_ld32-white", "B2_T8_C8_P4_ld4-drop_lo", "B4_T32_C16_P1_ld1-time_shift"],
    "shift_sign": ["B2_T50_C256_P25_ld32-time_shift", "B3_T15_C40_P5_ld32-shift_pad"],
    "tail_reuses_lane0": ["B2_T12_C6_P3_ld4-white", "B2_T12_C6_P3_ld4-mask_full"],
    "span_len_off_by_one": ["B2_T8_C8_P4_ld4-spans8", "B2_T12_C6_P3_ld4-spans8"],
}


def test_every_defect_is_listed():
    assert sorted(DEFECT_CASES) == sorted(AR.DEFECTS)


@pytest.mark.parametrize("defect", AR.DEFECTS)
def test_defect_breaks_the_bound(defect):
    for cid in DEFECT_CASES[defect]:
        c = AC.BY_ID[cid]
        x = c.x()
        ref, bnd = AR.bound(x, c.cfg, c.words, c.P, c.ldp)
        got = AR.forward(x, c.cfg, c.words, c.P, c.ldp, defect=defect)
        bad = np.abs(got - ref) > bnd + AR.half_ulp(ref, "bf16")             # the wider of the two bounds
        assert float(np.mean(bad)) > 0.05, (defect, cid, float(np.mean(bad)))


def test_argument_validation_needs_no_gpu():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1

    def go(B=2, T=8, C=8, P=4, ldp=4, dtype=_lib.FK_F32, x=64, tok=64, words=64, nocfg=False, **knobs):
        k = dict(white_sd=0.5, offset_sd=0.0, chan_drop_p=0.0, time_shift=0, n_time_masks=0, time_mask_len=0, keep_padding=1)
        k.update(knobs)
        cfg = _lib.AugmentCfg(k["white_sd"], k["offset_sd"], k["chan_drop_p"], k["time_shift"], k["n_time_masks"], k["time_mask_len"], k["keep_padding"], 0)
        return lib.fk_augment_patchify(x, tok, B, T, C, P, ldp, None if nocfg else ctypes.byref(cfg), words, dtype, None)

    assert go(x=None) == EINVAL and b"null" in lib.fk_last_error()
    assert go(tok=None) == EINVAL and go(words=None) == EINVAL and go(nocfg=True) == EINVAL and b"null" in lib.fk_last_error()
    assert go(T=10) == EINVAL and b"T % P" in lib.fk_last_error()
    assert go(ldp=3) == EINVAL and b"ldp >= P" in lib.fk_last_error()
    assert go(B=0) == EINVAL and go(C=0) == EINVAL
    assert go(T=64, P=64, C=256, ldp=64) == EINVAL and b"64 KiB" in lib.fk_last_error()
    for bad in (-0.1, float("inf"), float("nan")):
        assert go(white_sd=bad) == EINVAL and b"sd" in lib.fk_last_error()
        assert go(offset_sd=bad) == EINVAL and b"sd" in lib.fk_last_error()
    for bad in (-0.01, 1.0, 1.5, float("nan")):
        assert go(chan_drop_p=bad) == EINVAL and b"chan_drop_p" in lib.fk_last_error()
    for bad in (-1, 9):
        assert go(n_time_masks=bad) == EINVAL and b"n_time_masks" in lib.fk_last_error()
    for bad in (-1, 9):
        assert go(time_mask_len=bad) == EINVAL and b"time_mask_len" in lib.fk_last_error()
    for bad in (-1, 8):
        assert go(time_shift=bad) == EINVAL and b"time_shift" in lib.fk_last_error()
    assert go(dtype=7) == EINVAL and b"dtype" in lib.fk_last_error()
    assert go(x=66) == EINVAL and b"misaligned" in lib.fk_last_error()
    assert go(words=66) == EINVAL and b"misaligned" in lib.fk_last_error()
    assert go(B=1 << 40, T=1 << 20) == EINVAL and b"int32" in lib.fk_last_error()


def test_header_binding_and_wrappers_agree():
    from dataclasses import fields, is_dataclass
    from frankenstein_amd import _lib, build, engine, kernels
    from frankenstein_amd.models import brainformer as bf
    txt = (ROOT / "include" / "franken_hip.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    h = ctypes.CDLL(str(build.build(verbose=False)))
    proto = re.search(r"\bfk_augment_patchify\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["fk_augment_patchify"][1]) == 11 and hasattr(h, "fk_augment_patchify")
    assert "augment.hip" in build.SOURCES and h.fk_version() == 302
    struct = re.search(r"typedef struct fk_augment_cfg \{(.*?)\} fk_augment_cfg;", hdr, flags=re.S).group(1)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", struct)
    assert names == [f[0] for f in _lib.AugmentCfg._fields_] and ctypes.sizeof(_lib.AugmentCfg) == 32
    assert names[:7] == [f.name for f in fields(engine.AugmentConfig)]
    assert is_dataclass(engine.AugmentConfig) and engine.AugmentConfig.__dataclass_params__.frozen
    assert engine.AugmentConfig().keep_padding is True and not engine.AugmentConfig().active
    for k in ("white_sd", "offset_sd", "chan_drop_p", "time_shift"):
        assert engine.AugmentConfig(**{k: 1}).active
    assert not engine.AugmentConfig(n_time_masks=3).active and engine.AugmentConfig(n_time_masks=3, time_mask_len=2).active
    for fn in ("augment_patchify",):
        assert callable(getattr(kernels, fn))
    for fn in ("augment_words", "augment_begin", "augment_seed", "augment_signal"):
        assert callable(getattr(engine, fn))
    assert issubclass(bf.SignalAugment, torch.nn.Module) and not list(bf.SignalAugment(engine.AugmentConfig(white_sd=1.0)).parameters())
    assert "0xA0610000" in txt and "(wa >> 9) + 0.5" in txt                  # the rule is stated in the header
    assert "philox4x32_10" in (ROOT / "frankenstein_amd" / "csrc" / "fk_common.h").read_text()
    assert "void philox4x32_10" not in (ROOT / "frankenstein_amd" / "csrc" / "decode.hip").read_text()     # hoisted, not copied
    x = torch.ones(2, 4, 4)
    assert bf.SignalAugment(engine.AugmentConfig(white_sd=1.0)).eval()(x) is x                 # eval(): the identity, nothing launched
    assert bf.SignalAugment(engine.AugmentConfig()).train()(x) is x                            # all knobs zero: likewise


def test_augment_seed():
    from frankenstein_amd import engine as E
    seeds = [E.augment_seed(42, r) for r in range(8)]
    assert len(set(seeds)) == 8 and seeds[0] == 42
    for s0 in (0, 42, 2 ** 63 - 1, 0xFFFFFFFFFFFFFFFF):
        for r in (0, 1, 7, 1023):
            s = E.augment_seed(s0, r)
            assert 0 <= s < 2 ** 31 and s == (s0 + 0x9E3779B9 * r) & 0x7FFFFFFF


def _tiny(**aug):
    from frankenstein_amd.models.brainformer import Config, MAEConfig
    enc = MAEConfig(window_size=32, n_electrodes=16, patch_size=4, dim=32, n_layers=1, head_dim=16, hidden_dim=64, n_heads=2, n_kv_heads=2,
                    n_dec_layers=1, decoder_dim=32, **aug)
    return enc, Config(encoder=enc, n_output_tokens=4, output_dim=8, dim=32, n_layers=1, head_dim=16, hidden_dim=64, n_heads=2, n_kv_heads=2)


def _tiny_simple(**aug):
    from frankenstein_amd.models.simple_mae import SimpleEncoderConfig, SimpleMAEConfig
    return (SimpleEncoderConfig(block_size=16, patch_size=8, n_layers=1, dim=32, hidden_dim=64, head_dim=16, n_heads=2, n_kv_heads=2, **aug),
            SimpleMAEConfig(n_layers=1, dim=32, hidden_dim=64, head_dim=16, n_heads=2, n_kv_heads=2))


def test_config_fields_and_state_dict_keys():
    from dataclasses import fields
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models import simple_mae as sm
    names = ("aug_white_sd", "aug_offset_sd", "aug_chan_drop", "aug_time_shift", "aug_time_masks", "aug_time_mask_len")
    for cls in (bf.MAEConfig, sm.SimpleEncoderConfig):
        have = {f.name: f.default for f in fields(cls)}
        assert all(have[n] == 0 for n in names), cls
    on = dict(aug_white_sd=0.5, aug_offset_sd=0.2, aug_chan_drop=0.1, aug_time_masks=2, aug_time_mask_len=4)
    enc0, cfg0 = _tiny()
    enc1, cfg1 = _tiny(**on)
    for make in ((lambda e, c: bf.Encoder(e)), (lambda e, c: bf.BrainFormer(c)), (lambda e, c: bf.MAE(e))):
        m0, m1 = make(enc0, cfg0), make(enc1, cfg1)
        assert set(m0.state_dict()) == set(m1.state_dict()) and not any("aug" in k for k in m1.state_dict())
        assert [n for n, _ in m0.named_parameters()] == [n for n, _ in m1.named_parameters()]
        assert [n for n, _ in m0.named_buffers()] == [n for n, _ in m1.named_buffers()]
    e1 = bf.Encoder(enc1)
    assert e1.augment.active and e1.augment.white_sd == 0.5 and e1.augment.n_time_masks == 2 and not bf.Encoder(enc0).augment.active
    assert e1.augment_active() and not e1.eval().augment_active() and not bf.Encoder(enc0).augment_active()
    s0, s1 = sm.SimpleMAE(*_tiny_simple()), sm.SimpleMAE(*_tiny_simple(**on))
    assert set(s0.state_dict()) == set(s1.state_dict()) and s1.encoder.augment.active and not s0.encoder.augment.active


def test_mae_refuses_a_shift():
    from frankenstein_amd.models import brainformer as bf
    from frankenstein_amd.models import simple_mae as sm
    enc, cfg = _tiny(aug_time_shift=2)
    with pytest.raises(ValueError, match="aug_time_shift"):
        bf.MAE(enc)
    with pytest.raises(ValueError, match="aug_time_shift"):
        sm.SimpleMAE(*_tiny_simple(aug_time_shift=1))
    assert bf.Encoder(enc).augment.time_shift == 2 and bf.BrainFormer(cfg).encoder.augment.active     # the supervised models may shift
