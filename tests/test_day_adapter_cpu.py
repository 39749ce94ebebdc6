"""Host-side checks of the per-session input adapter (csrc/dayadapt.hip, engine.DayPatchify, models.brainformer.DayAdapter):
  * the numpy float64 restatement (tests/day_adapter_ref.py) equals torch's float64 einsum / autograd composition on every case;
  * each planted defect breaks the bound of tests/test_day_adapter_gpu.py on a named case (so that test would catch it);
  * argument validation returns FK_EINVAL without a GPU; header, binding and wrappers agree for the new symbols;
  * n_days = 0 leaves the state-dict key set of Encoder, BrainFormer and MAE unchanged, n_days = 3 adds exactly the two keys."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import day_adapter_cases as DC
from tests import day_adapter_ref as DR

ROOT = Path(__file__).resolve().parents[1]
SMALL = [c for c in DC.CASES]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_restatement_equals_torch_float64(case):
    x, day, delta, bias, d_tok = case.inputs()
    ref = (DR.forward(x, day, delta, bias, case.P, case.ldp), *DR.backward(x, day, d_tok, case.P, case.n_days))
    t64 = DR.torch_composition(x, day, delta, bias, d_tok, case.P, case.ldp, torch.float64)
    for name, a, r in zip(("tok", "d_delta", "d_bias"), t64, ref):
        scale = max(1.0, float(np.max(np.abs(r))))
        assert a.shape == r.shape
        assert float(np.max(np.abs(a - r))) <= 1e-12 * scale * case.T * case.B, name
    assert np.all(ref[0][:, :, case.P:] == 0.0)
    for dt in case.dtypes:                     # the rounded form: within half an ulp of the exact one, and a value of the dtype
        r = DR.forward(x, day, delta, bias, case.P, case.ldp, dtype=dt)
        assert np.all(np.abs(r - ref[0]) <= DR.half_ulp(ref[0], dt) * (1 + 1e-9))
        assert np.array_equal(DR.round_to(r, dt), r)


def test_route_shapes_take_the_routes_they_name():
    """the shapes added for the forward's 64- and 128-row workgroups do take them; the issue's shapes all take 32 rows"""
    assert [DC.fwd_rows(*s[:3]) for s in DC.ROUTE_SHAPES] == [64, 128, 128, 64, 64]
    assert {DC.fwd_rows(*s[:3]) for s in DC.SHAPES} == {32}
    assert all(s[1] % s[3] == 0 and s[4] >= s[3] for s in DC.SHAPES + DC.ROUTE_SHAPES)
    assert DC.fwd_rows(32, 600, 256) == 64


# defect -> (case id, tensor it must break: 0 tok, 1 d_delta, 2 d_bias)
DEFECT_CASES = {
    "delta_transposed": [("B4_T32_C16_P4_ld32_D3-different", 0), ("B4_T32_C16_P4_ld32_D3-different", 1)],
    "first_day_for_all": [("B5_T50_C256_P25_ld32_D24-mixed", 0), ("B5_T50_C256_P25_ld32_D24-mixed", 1), ("B3_T8_C8_P4_ld4_D2-different", 2)],
    "bias_dropped": [("B3_T8_C8_P4_ld4_D2-same", 0), ("B2_T200_C64_P25_ld32_D4-same", 2)],
    "day_clamped": [("B5_T50_C256_P25_ld32_D24-mixed", 0), ("B2_T15_C40_P5_ld32_D2-outrange", 1), ("B2_T15_C40_P5_ld32_D2-outrange", 2)],
    "pc_swapped": [("B2_T15_C40_P5_ld32_D2-same", 1), ("B2_T200_C64_P25_ld32_D4-different", 2)],
    "absent_unwritten": [("B4_T32_C16_P4_ld32_D3-absent", 1), ("B5_T50_C256_P25_ld32_D24-mixed", 2)],
}


def test_every_defect_is_listed():
    assert sorted(DEFECT_CASES) == sorted(DR.DEFECTS)


@pytest.mark.parametrize("defect", DR.DEFECTS)
def test_defect_breaks_the_bound(defect):
    for cid, which in DEFECT_CASES[defect]:
        case = DC.BY_ID[cid]
        x, day, delta, bias, d_tok = case.inputs()
        ref, bnd = DR.bounds(x, day, delta, bias, d_tok, case.P, case.ldp)
        if which == 0:
            got = DR.forward(x, day, delta, bias, case.P, case.ldp, defect=defect)
            lim = bnd[0] + DR.half_ulp(ref[0], "bf16")             # the wider of the two forward bounds
        else:
            got = DR.backward(x, day, d_tok, case.P, case.n_days, defect=defect, prefill=np.nan)[which - 1]
            lim = bnd[which]
        ok = np.abs(got - ref[which]) <= lim                        # NaN compares False
        assert not np.all(ok), (defect, cid, which)
        assert float(np.mean(~ok)) > 0.05, (defect, cid, which)     # gross: not one stray element


def test_argument_validation_needs_no_gpu():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    EINVAL = -1

    def fwd(B=2, T=8, C=8, P=4, ldp=4, n_days=2, dtype=_lib.FK_F32, x=64, day=64, delta=64, bias=64, tok=64):
        return lib.fk_day_adapter_fwd(x, day, delta, bias, tok, B, T, C, P, ldp, n_days, dtype, None)

    def bwd(B=2, T=8, C=8, P=4, ldp=4, n_days=2, x=64, day=64, d_tok=64, d_delta=64, d_bias=64, ws=64, nbytes=1 << 30):
        return lib.fk_day_adapter_bwd(x, day, d_tok, ldp, d_delta, d_bias, ws, nbytes, B, T, C, P, n_days, None)

    for f in (fwd, bwd):
        assert f(C=0) == EINVAL and b"envelope" in lib.fk_last_error()
        assert f(C=513) == EINVAL and b"envelope" in lib.fk_last_error()
        assert f(T=10) == EINVAL and b"T % P" in lib.fk_last_error()
        assert f(ldp=3) == EINVAL and b"ldp >= P" in lib.fk_last_error()
        assert f(n_days=0) == EINVAL and b"n_days" in lib.fk_last_error()
        assert f(B=0) == EINVAL
        assert f(B=1 << 20, T=1 << 12, C=512) == EINVAL and b"int32" in lib.fk_last_error()
        assert f(x=None) == EINVAL and b"null" in lib.fk_last_error()
        assert f(x=66) == EINVAL and b"misaligned" in lib.fk_last_error()
        assert f(day=68) == EINVAL and b"misaligned" in lib.fk_last_error()
    assert fwd(dtype=7) == EINVAL and b"dtype" in lib.fk_last_error()
    assert fwd(tok=None) == EINVAL and fwd(delta=None) == EINVAL and fwd(bias=None) == EINVAL
    assert bwd(d_delta=None) == EINVAL and bwd(d_bias=None) == EINVAL and bwd(d_tok=None) == EINVAL
    need = lib.fk_day_adapter_bwd_workspace_bytes(2, 8, 8, 4, 2)
    assert need >= 2 * (8 * 8 + 8) * 4
    assert bwd(nbytes=need - 1) == EINVAL and b"workspace" in lib.fk_last_error()
    assert bwd(ws=None) == EINVAL and b"workspace" in lib.fk_last_error()
    assert bwd(n_days=70000) == EINVAL
    # the workspace grows with the number of time slices, which comes from the shape alone
    assert lib.fk_day_adapter_bwd_workspace_bytes(32, 600, 256, 25, 24) == 32 * 2 * (256 * 256 + 256) * 4
    assert lib.fk_day_adapter_bwd_workspace_bytes(1, 4, 512, 4, 1) == (512 * 512 + 512) * 4


def test_header_binding_and_wrappers_agree():
    from frankenstein_amd import _lib, build, kernels, engine
    import ctypes
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "franken_hip.h").read_text(), flags=re.S)
    h = ctypes.CDLL(str(build.build(verbose=False)))
    for name in ("fk_day_adapter_fwd", "fk_day_adapter_bwd", "fk_day_adapter_bwd_workspace_bytes"):
        proto = re.search(r"\b%s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(h, name)
    assert "dayadapt.hip" in build.SOURCES
    assert _lib.SIGNATURES["fk_day_adapter_bwd_workspace_bytes"][0] is ctypes.c_size_t
    for fn in ("day_adapter_fwd", "day_adapter_bwd"):
        assert callable(getattr(kernels, fn))
    for cls in ("DayPatchify", "PatchEmbedTok", "MaskedPatchEmbedTok"):
        assert issubclass(getattr(engine, cls), torch.autograd.Function)
    txt = (ROOT / "include" / "franken_hip.h").read_text()
    assert "x[b, t, :] + x[b, t, :] @ delta[d] + bias[d]" in txt      # the rule is stated in the header


def test_day_ids_forms():
    from frankenstein_amd import engine as E
    cpu = torch.device("cpu")
    assert E.day_ids(None, 3, cpu) is None
    assert E.day_ids(2, 3, cpu).tolist() == [2, 2, 2] and E.day_ids(2, 3, cpu).dtype == torch.int64
    assert E.day_ids(torch.tensor([1, -1, 0], dtype=torch.int32), 3, cpu).tolist() == [1, -1, 0]
    t = torch.tensor([4, 5], dtype=torch.int64)
    assert E.day_ids(t, 2, cpu).data_ptr() == t.data_ptr()              # already in the kernels' form: no copy
    with pytest.raises(ValueError):
        E.day_ids(torch.tensor([1, 2]), 3, cpu)
    with pytest.raises(TypeError):
        E.day_ids(torch.tensor([1.0, 2.0, 3.0]), 3, cpu)


def _tiny(n_days):
    from frankenstein_amd.models.brainformer import Config, MAEConfig
    enc = MAEConfig(window_size=32, n_electrodes=16, patch_size=4, dim=32, n_layers=1, head_dim=16, hidden_dim=64, n_heads=2, n_kv_heads=2,
                    n_dec_layers=1, decoder_dim=32, n_days=n_days)
    return enc, Config(encoder=enc, n_output_tokens=4, output_dim=8, dim=32, n_layers=1, head_dim=16, hidden_dim=64, n_heads=2, n_kv_heads=2)


def test_state_dict_keys():
    from dataclasses import fields
    from frankenstein_amd.models import brainformer as bf
    assert fields(bf.MAEConfig)[-1].name == "n_days" and bf.MAEConfig().n_days == 0
    enc0, cfg0 = _tiny(0)
    enc3, cfg3 = _tiny(3)
    for make, prefix in ((lambda e, c: bf.Encoder(e), ""), (lambda e, c: bf.BrainFormer(c), "encoder."), (lambda e, c: bf.MAE(e), "encoder.")):
        m0, m3 = make(enc0, cfg0), make(enc3, cfg3)
        k0, k3 = set(m0.state_dict()), set(m3.state_dict())
        assert not any("day_adapter" in k for k in k0)
        assert not any("day_adapter" in n for n, _ in m0.named_parameters())
        assert k3 - k0 == {prefix + "day_adapter.delta", prefix + "day_adapter.bias"} and k0 <= k3
        sd = m3.state_dict()
        assert sd[prefix + "day_adapter.delta"].shape == (3, 16, 16) and sd[prefix + "day_adapter.bias"].shape == (3, 16)
        assert float(sd[prefix + "day_adapter.delta"].abs().max()) == 0.0 and float(sd[prefix + "day_adapter.bias"].abs().max()) == 0.0
    with pytest.raises(ValueError):
        bf.DayAdapter(0, 16)
    with pytest.raises(ValueError):
        bf.DayAdapter(2, 513)
    ad = bf.DayAdapter(3, 4)
    with torch.no_grad():
        ad.delta[1].fill_(2.0)
        ad.bias[1].fill_(3.0)
    ad.copy_day(1, 2)
    assert torch.equal(ad.delta[2], ad.delta[1]) and torch.equal(ad.bias[2], ad.bias[1]) and float(ad.delta.detach()[0].abs().max()) == 0.0
    with pytest.raises(IndexError):
        ad.copy_day(0, 3)
