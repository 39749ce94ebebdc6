"""Low-rank adapters without a GPU: the float64 restatement of tests/lora_ref.py against torch.autograd (a derivation check, exact up to
float64 rounding), the fk_lora_route table over the envelope and just outside it, and the host-side refusals of the entry points (no
launch happens on an invalid shape, so they can be asked here)."""
import numpy as np
import pytest
import torch

from frankenstein_amd._lib import LORA_R32, LORA_R64          # the binding of csrc/lora.hip: without it nothing here means anything
from tests import lora_ref as LR


@pytest.mark.parametrize("q_cols,q_scale", [(0, 1.0), (5, 0.125)])
def test_restatement_matches_autograd_in_float64(q_cols, q_scale):
    g = torch.Generator().manual_seed(3)
    M, N, Kd, r, s = 7, 12, 10, 4, 0.75
    x, A, B, res, dy = (torch.randn(sh, generator=g, dtype=torch.float64) for sh in ((M, Kd), (r, Kd), (N, r), (M, N), (M, N)))
    xt, At, Bt = (v.clone().requires_grad_(True) for v in (x, A, B))
    cs = torch.ones(N, dtype=torch.float64)
    cs[:q_cols] = q_scale
    out = res + s * cs * ((xt @ At.t()) @ Bt.t())                       # the plain formula
    out.backward(dy)
    u_ref, out_ref = LR.forward(x.numpy(), A.numpy(), B.numpy(), s, res.numpy(), q_cols, q_scale)
    du, dx, dA, dB = LR.backward(x.numpy(), A.numpy(), B.numpy(), s, dy.numpy(), q_cols, q_scale)
    close = lambda a, b: np.allclose(a, b, rtol=1e-13, atol=1e-13)
    assert close(out_ref, out.detach().numpy()) and close(u_ref, (x @ A.t()).numpy())
    assert close(dx, xt.grad.numpy()) and close(dA, At.grad.numpy()) and close(dB, Bt.grad.numpy())
    assert close(du, ((dy * cs) @ B).numpy())
    # the transposed-role call is the same forward: du and the data gradient from B^T and A^T
    du2, dh = LR.forward((dy * cs).numpy(), B.t().numpy(), A.t().numpy(), s, np.zeros((M, Kd)))
    assert close(du2, du) and close(dh, dx)
    # merged weight: x W'^T is the adapted product
    W = torch.randn(N, Kd, generator=g, dtype=torch.float64)
    assert close(x.numpy() @ LR.merge(W.numpy(), A.numpy(), B.numpy(), s).T, (x @ W.t() + s * (x @ A.t()) @ B.t()).numpy())


def test_rounded_evaluation_and_exact_operands():
    x, A, B, res, dy = LR.exact_operands(33, 72, 768, 16, seed=1)
    u, out = LR.forward(x, A, B, 0.5, res)
    for dt in ("bf16", "fp32"):
        assert all(LR.representable(v, dt) for v in (x, A, B, res, dy, u))
        u_c, out_c = LR.rounded_forward(x, A, B, 0.5, dt, res)
        assert np.array_equal(u_c, u)                                   # exact operands: the rounded evaluation IS the float64 one
        assert np.array_equal(out_c, out) or dt == "bf16"
    assert not LR.representable(np.array([1.0 + 2.0 ** -9]), "bf16")


def test_route_table():
    from frankenstein_amd import _lib, kernels as K
    BFd, F32d = _lib.FK_BF16, _lib.FK_F32
    for dt in (BFd, F32d):
        for r in range(4, 65, 4):
            assert K.lora_route(1824, 2304, 768, r, dt) == (_lib.LORA_R32 if r <= 32 else _lib.LORA_R64), (r, dt)
        for r in (0, 2, 6, 68, -4, 65):
            assert K.lora_route(1824, 2304, 768, r, dt) == -1, (r, dt)
        assert K.lora_route(1, 8, 8, 4, dt) == _lib.LORA_R32
        assert K.lora_route(0, 8, 8, 4, dt) == -1
        for big in (dict(M=1 << 31), dict(N=1 << 31), dict(Kd=1 << 31)):
            kw = dict(M=8, N=8, Kd=8)
            kw.update(big)
            assert K.lora_route(kw["M"], kw["N"], kw["Kd"], 4, dt) == -1, big
        assert K.lora_route((1 << 31) - 1, (1 << 31) - 8, (1 << 31) - 8, 64, dt) == _lib.LORA_R64
    assert K.lora_route(8, 8, 12, 4, BFd) == -1 and K.lora_route(8, 8, 12, 4, F32d) == _lib.LORA_R32        # K = 12: fp32 only
    assert K.lora_route(8, 4, 8, 4, BFd) == -1 and K.lora_route(8, 4, 8, 4, F32d) == _lib.LORA_R32          # N = 4: fp32 only
    assert K.lora_route(8, 8, 6, 4, F32d) == -1 and K.lora_route(8, 2, 8, 4, F32d) == -1
    assert K.lora_route(8, 8, 8, 4, 7) == -1
    assert K.lora_route(8, 8, 8, 4, torch.bfloat16) == _lib.LORA_R32


def _tiny_gpt(**kw):
    from frankenstein_amd.models import gpt2_model as g2
    cfg = dict(block_size=64, vocab_size=96, n_layer=2, n_head=2, n_embd=128, dropout=0.0, bias=True)
    cfg.update(kw)
    return g2.GPT(g2.GPTConfig(**cfg))


def test_add_lora_registers_the_adapters_and_freezes_the_rest():
    import math
    g = _tiny_gpt()
    base_keys = list(g.state_dict())
    assert g.lora_config() is None and g.lora_state_dict() == {}
    g.add_lora(rank=8, alpha=16.0)
    lin = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
    want = [f"transformer.h.{i}.{l}.lora_{ab}" for i in range(2) for l in lin for ab in "AB"]
    trainable = [n for n, p in g.named_parameters() if p.requires_grad]
    assert trainable == want and list(g.lora_state_dict()) == want
    assert [k for k in g.state_dict() if "lora_" not in k] == base_keys           # the base keys are untouched
    assert all(not p.requires_grad for n, p in g.named_parameters() if "lora_" not in n)
    shapes = {"attn.c_attn": (384, 128), "attn.c_proj": (128, 128), "mlp.c_fc": (512, 128), "mlp.c_proj": (128, 512)}
    sd = g.lora_state_dict()
    for l, (n_out, n_in) in shapes.items():
        a, b = sd[f"transformer.h.1.{l}.lora_A"], sd[f"transformer.h.1.{l}.lora_B"]
        assert a.shape == (8, n_in) and b.shape == (n_out, 8) and a.dtype == b.dtype == torch.float32
        assert float(b.abs().max()) == 0.0 and 0.0 < float(a.abs().max()) <= 1.0 / math.sqrt(n_in)       # nn.Linear's Kaiming-uniform bound
    assert g.transformer.h[0].attn.c_attn.lora_scale == 2.0
    assert g.lora_config() == dict(rank=8, alpha=16.0, targets=("c_attn", "attn.c_proj", "c_fc", "mlp.c_proj"))
    with pytest.raises(RuntimeError):
        g.add_lora()
    for bad in (dict(rank=6), dict(rank=68), dict(rank=2), dict(targets=("lm_head",))):
        with pytest.raises(ValueError):
            _tiny_gpt().add_lora(**bad)
    h = _tiny_gpt().add_lora(rank=4, targets=("c_fc",))
    assert [n for n, p in h.named_parameters() if p.requires_grad] == [f"transformer.h.{i}.mlp.c_fc.lora_{ab}" for i in range(2) for ab in "AB"]


def test_adapter_state_round_trips(tmp_path):
    from frankenstein_amd.utils import train_utils as tu
    torch.manual_seed(0)
    g = _tiny_gpt().add_lora(rank=12, alpha=6.0, targets=("c_attn", "mlp.c_proj"))
    with torch.no_grad():
        for p in g.lora_state_dict().values():
            p.copy_(torch.randn_like(p))
    sd = {k: v.clone() for k, v in g.lora_state_dict().items()}
    h = _tiny_gpt().add_lora(rank=12, alpha=6.0, targets=("c_attn", "mlp.c_proj"))
    h.load_lora_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in h.lora_state_dict().items())
    with pytest.raises(KeyError):
        _tiny_gpt().add_lora(rank=12, targets=("c_fc",)).load_lora_state_dict(sd)
    with pytest.raises(ValueError):
        _tiny_gpt().add_lora(rank=8, targets=("c_attn", "mlp.c_proj")).load_lora_state_dict(sd)
    tu.save_lora(g, tmp_path / "a.safetensors")
    import safetensors
    with safetensors.safe_open(str(tmp_path / "a.safetensors"), framework="pt") as f:
        assert f.metadata() == {"lora_rank": "12", "lora_alpha": "6.0", "lora_targets": "c_attn,mlp.c_proj"} and sorted(f.keys()) == sorted(sd)
    fresh = _tiny_gpt()
    assert tu.load_lora(fresh, tmp_path / "a.safetensors") == dict(rank=12, alpha=6.0, targets=("c_attn", "mlp.c_proj"))
    assert all(torch.equal(v, sd[k]) for k, v in fresh.lora_state_dict().items()) and fresh.transformer.h[0].attn.c_attn.lora_scale == 0.5
    assert all(p.requires_grad == ("lora_" in n) for n, p in fresh.named_parameters())
    with pytest.raises(ValueError):
        tu.load_lora(_tiny_gpt().add_lora(rank=8), tmp_path / "a.safetensors")
    with pytest.raises(RuntimeError):
        tu.save_lora(_tiny_gpt(), tmp_path / "b.safetensors")


def test_wgrad_path_skip_and_optimizer_groups():
    from frankenstein_amd import engine as E
    from frankenstein_amd.utils import train_utils as tu
    assert E.wgrad_path([False], requires_grad=[False]) == "skip" and E.wgrad_path([True, True], True, True, True, requires_grad=[False, False]) == "skip"
    assert E.wgrad_path([False, False], requires_grad=[False, True]) == "tensors"
    assert E.wgrad_path([True], requires_grad=[True]) == "split_add" and E.wgrad_path([True], adjacent=True, requires_grad=None) == "adjacent"
    assert E.wgrad_path([False]) == "tensors" and E.wgrad_path([True, True], True, True) == "swiglu_slab"         # existing calls keep their answers
    g = _tiny_gpt().add_lora(rank=8)
    g.transformer.ln_f.weight.requires_grad_(True)                                # a caller may re-enable some
    g.transformer.h[0].mlp.c_fc.weight.requires_grad_(True)
    groups = tu.decay_groups(g, 0.1)
    ids = lambda ps: {id(p) for p in ps}
    frozen = ids(p for p in g.parameters() if not p.requires_grad)
    lora = ids(g.lora_state_dict().values()) | ids(p for n, p in g.named_parameters() if "lora_" in n)
    assert not (ids(groups[0]["params"]) | ids(groups[1]["params"])) & frozen
    assert ids(groups[0]["params"]) == {id(g.transformer.h[0].mlp.c_fc.weight)} and groups[0]["weight_decay"] == 0.1
    assert ids(groups[1]["params"]) == ids(p for n, p in g.named_parameters() if "lora_" in n) | {id(g.transformer.ln_f.weight)}
    assert groups[1]["weight_decay"] == 0.0 and lora
    opt = g.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu")
    assert not ids(p for grp in opt.param_groups for p in grp["params"]) & frozen
    assert sum(len(grp["params"]) for grp in opt.param_groups) == 16 + 2


def test_entry_points_refuse_the_envelope_on_the_host():
    from frankenstein_amd import _lib
    lib = _lib.lib()
    p, BFd, F32d = 4096, _lib.FK_BF16, _lib.FK_F32                       # a fake, aligned pointer: nothing is launched
    fwd = lambda M=8, N=8, Kd=8, r=4, dt=BFd, ldx=8, ldo=8: lib.fk_lora_fwd(p, ldx, p, p, M, N, Kd, r, 1.0, 0, 1.0, None, 0, p, p, ldo, dt, None)
    wg = lambda M=8, N=8, Kd=8, r=4, dt=BFd: lib.fk_lora_wgrad(p, p, p, p, M, N, Kd, r, 1.0, p, p, 0, dt, None, 0, None)
    mg = lambda N=8, Kd=8, r=4, dt=BFd: lib.fk_lora_merge(p, p, p, N, Kd, r, 1.0, p, Kd, dt, None)
    for kw in (dict(r=0), dict(r=2), dict(r=6), dict(r=68), dict(Kd=12), dict(N=4), dict(dt=7), dict(Kd=6, dt=F32d)):
        assert fwd(**kw) == -1 and b"fk_lora_fwd: outside the envelope" in lib.fk_last_error(), kw
        assert wg(**kw) == -1 and b"fk_lora_wgrad: outside the envelope" in lib.fk_last_error(), kw
        assert mg(**kw) == -1 and b"fk_lora_merge: outside the envelope" in lib.fk_last_error(), kw
    assert fwd(M=0) == -1 and wg(M=0) == -1
    assert fwd(ldx=0) == -1 and b"leading dimensions" in lib.fk_last_error()
    assert fwd(ldo=4) == -1 and b"leading dimensions" in lib.fk_last_error()
    assert fwd(Kd=8, ldx=12) == -1 and b"16 bytes" in lib.fk_last_error()
    assert wg(M=65) == -1 and b"workspace too small" in lib.fk_last_error()
    assert lib.fk_lora_wgrad_workspace_bytes(64, 72, 768, 16) == 0
    assert lib.fk_lora_wgrad_workspace_bytes(1824, 2304, 768, 16) == 29 * (2304 * 16 + 16 * 768) * 4
