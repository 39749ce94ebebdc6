"""Host side of the grouped optimizer (no GPU): the two entry points in the header and the binding, their argument checks, the pure
function that turns (arena layout, groups, reached flags, lags, step) into the segment / slot tables of fk_adamw_step_groups, the
constructor's refusals, and the reference's decay / no-decay split."""
import random
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW = ("fk_adamw_step_groups", "fk_grad_sumsq")


@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_and_binding_carry_both_entry_points(lib):
    from frankenstein_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "franken_hip.h").read_text(), flags=re.S)
    for name in NEW:
        proto = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S)
        assert proto is not None, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.fk_version() == 302
    assert re.search(r"#define FK_ADAMW_MAX_SLOTS (\d+)", hdr).group(1) == str(_lib.ADAMW_MAX_SLOTS) == "16"
    assert re.search(r"#define FK_GRAD_SUMSQ_MAX_BLOCKS (\d+)", hdr).group(1) == str(_lib.GRAD_SUMSQ_MAX_BLOCKS) == "1024"
    import ctypes
    assert ctypes.sizeof(_lib.AdamwGroup) == 48          # fk_adamw_group: five doubles and an int64


def test_bad_arguments_are_refused_before_any_launch(lib):
    from frankenstein_amd import _lib
    slots = (_lib.AdamwGroup * 17)(*[_lib.AdamwGroup(1e-3, 0.9, 0.999, 1e-8, 0.0, 1) for _ in range(17)])
    A = 4096                                              # a non-null, 16-byte aligned address; nothing is launched, so nothing reads it

    def step(p=A, g=A, segs=A, nseg=1, groups=slots, nslots=1, max_norm=0.0, partials=None, npartials=0, norm_out=None):
        return lib.fk_adamw_step_groups(p, g, A, A, 1024, segs, nseg, groups, nslots, 0.0, 1.0, 0, max_norm, partials, npartials, norm_out, None)

    assert step(segs=None) == -1 and b"fk_adamw_step_groups: null pointer" in lib.fk_last_error()
    assert step(groups=None) == -1 and b"null pointer" in lib.fk_last_error()
    assert step(nslots=0) == -1 and b"nslots = 0" in lib.fk_last_error()
    assert step(nslots=17) == -1 and b"nslots = 17" in lib.fk_last_error()
    assert step(p=A + 4) == -1 and b"16-byte aligned" in lib.fk_last_error()
    assert step(g=A + 8) == -1 and b"16-byte aligned" in lib.fk_last_error()
    assert step(nseg=0) == -1 and b"nseg = 0" in lib.fk_last_error()
    assert step(max_norm=-1.0) == -1 and b"max_norm" in lib.fk_last_error()
    assert step(max_norm=1.0) == -1 and b"partials" in lib.fk_last_error()               # a norm clip without the partial sums
    assert step(max_norm=1.0, partials=A, npartials=1025, norm_out=A) == -1 and b"partials" in lib.fk_last_error()
    bad = (_lib.AdamwGroup * 1)(_lib.AdamwGroup(1e-3, 0.9, 0.999, 1e-8, 0.0, 0))
    assert step(groups=bad) == -1 and b"step 0" in lib.fk_last_error()

    def sumsq(g=A, segs=A, nseg=1, partials=A, npartials=1024):
        return lib.fk_grad_sumsq(g, 1024, segs, nseg, partials, npartials, None)

    assert sumsq(segs=None) == -1 and b"fk_grad_sumsq: null pointer" in lib.fk_last_error()
    assert sumsq(partials=None) == -1 and b"null pointer" in lib.fk_last_error()
    assert sumsq(g=A + 4) == -1 and b"16-byte aligned" in lib.fk_last_error()
    assert sumsq(nseg=0) == -1 and b"nseg = 0" in lib.fk_last_error()
    assert sumsq(npartials=0) == -1 and sumsq(npartials=1025) == -1 and b"npartials = 1025" in lib.fk_last_error()


def _brute(offsets, sizes, group_of, touched, lag, t):
    """element -> (group, step) for every element of a reached parameter (its padding to 4 included), by the definition"""
    want = {}
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        if touched[i]:
            for e in range(o, o + (n + 3) // 4 * 4):
                want[e] = (group_of[i], t - (lag[i] if lag is not None else 0))
    return want


def _layout(rng, nparams):
    sizes = [rng.choice([1, 3, 4, 5, 7, 8, 12, 64, 129, 333]) for _ in range(nparams)]
    offsets, off = [], 0
    for n in sizes:
        offsets.append(off)
        off += (n + 3) // 4 * 4
    return offsets, sizes, off


@pytest.mark.parametrize("seed", range(12))
def test_table_builder_against_a_per_element_map(seed):
    from frankenstein_amd.utils import train_utils as tu
    rng = random.Random(seed)
    offsets, sizes, total = _layout(rng, 40)
    ngroups = rng.choice([1, 2, 3, 5])
    group_of = [rng.randrange(ngroups) for _ in sizes]
    touched = [rng.random() < (0.5 if seed % 3 else 0.9) for _ in sizes]
    lag = None if seed % 4 == 0 else [rng.choice([0, 0, 0, 1, 2, 7]) if seed % 2 else rng.randrange(30) for _ in sizes]
    t = 31
    frozen = (list(offsets), list(sizes), list(group_of), list(touched), None if lag is None else list(lag))
    launches = tu.adamw_tables(offsets, sizes, group_of, touched, lag, t)
    assert (offsets, sizes, group_of, touched, lag) == frozen                    # a pure function
    want = _brute(offsets, sizes, group_of, touched, lag, t)
    got, all_keys = {}, []
    for segs, slots in launches:
        assert 1 <= len(slots) <= 16 and len(set(slots)) == len(slots) and segs
        all_keys += slots
        assert sorted({s for _, _, s in segs}) == list(range(len(slots)))        # every slot of a launch is used
        prev_end, prev_slot = -1, None
        for b, e, s in segs:
            assert b % 4 == 0 and e % 4 == 0 and 0 <= b < e <= total
            assert b >= prev_end                                                 # sorted, disjoint
            assert not (b == prev_end and s == prev_slot)                        # merged: no two adjacent segments of one slot
            prev_end, prev_slot = e, s
            for el in range(b, e):
                assert el not in got                                             # covered once, over all launches
                got[el] = slots[s]
    assert got == want                                  # every reached element by the right (group, step), no other element
    assert len(set(all_keys)) == len(all_keys) == len(set(want.values()))        # launches carry disjoint sets of (group, step) pairs
    assert len(launches) == (len(all_keys) + 15) // 16


def test_table_builder_merges_and_splits():
    from frankenstein_amd.utils import train_utils as tu
    offsets, sizes = [0, 4, 12, 20, 24], [3, 8, 5, 4, 2]
    # alternating groups: one segment per parameter; one group: one segment over everything
    assert tu.adamw_tables(offsets, sizes, [0, 1, 0, 1, 0], [True] * 5, None, 7) == [
        ([(0, 4, 0), (4, 12, 1), (12, 20, 0), (20, 24, 1), (24, 28, 0)], [(0, 7), (1, 7)])]
    assert tu.adamw_tables(offsets, sizes, [0] * 5, [True] * 5, None, 7) == [([(0, 28, 0)], [(0, 7)])]
    # parameter 2 not reached: a hole; parameter 3 sat out two steps: its own slot although it shares the group
    assert tu.adamw_tables(offsets, sizes, [0] * 5, [True, True, False, True, True], [0, 0, 4, 2, 0], 9) == [
        ([(0, 12, 0), (20, 24, 1), (24, 28, 0)], [(0, 9), (0, 7)])]
    assert tu.adamw_tables(offsets, sizes, [0] * 5, [False] * 5, None, 3) == []
    # 40 parameters that each sat out another number of steps: 40 pairs, three launches' worth under the cap of 16
    rng = random.Random(0)
    offs, szs, _ = _layout(rng, 40)
    got = tu.adamw_tables(offs, szs, [i % 2 for i in range(40)], [True] * 40, list(range(40)), 100)
    assert [len(slots) for _, slots in got] == [16, 16, 8] and [len(segs) for segs, _ in got] == [16, 16, 8]
    assert [slots[0] for _, slots in got] == [(0, 100), (0, 84), (0, 68)]
    # 5 (group, step) pairs under a cap of 2: three launches over disjoint parts of the table
    got = tu.adamw_tables(offsets, sizes, [0, 1, 2, 3, 4], [True] * 5, None, 1, max_slots=2)
    assert got == [([(0, 4, 0), (4, 12, 1)], [(0, 1), (1, 1)]), ([(12, 20, 0), (20, 24, 1)], [(2, 1), (3, 1)]), ([(24, 28, 0)], [(4, 1)])]


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(5, 7))
        self.b = torch.nn.Parameter(torch.zeros(7))
        self.frozen = torch.nn.Parameter(torch.zeros(3), requires_grad=False)


def test_constructor_refuses_bad_groups_and_two_clips():
    from frankenstein_amd.utils import train_utils as tu
    m = _Tiny()
    with pytest.raises(ValueError, match="already in a group"):
        tu.FusedAdamW(m, param_groups=[{'params': [m.w]}, {'params': [m.b, m.w]}])
    with pytest.raises(ValueError, match="already in a group"):
        tu.FusedAdamW(m, param_groups=[{'params': [m.w, m.w]}])
    with pytest.raises(ValueError, match="not a trainable parameter"):
        tu.FusedAdamW(m, param_groups=[{'params': [torch.nn.Parameter(torch.zeros(5, 7))]}])
    with pytest.raises(ValueError, match="not a trainable parameter"):
        tu.FusedAdamW(m, param_groups=[{'params': [m.frozen]}])
    with pytest.raises(ValueError, match="alternatives"):
        tu.FusedAdamW(m, grad_clip=1.0, grad_clip_norm=1.0)
    assert not hasattr(m.w, "_fk_arena")                # refused before the arena took the parameters over
    # the groups in torch's shape: the listed ones, then the rest as the default group from the constructor's arguments
    opt = tu.FusedAdamW(m, lr=1e-3, weight_decay=0.3, betas=(0.8, 0.9), grad_clip_norm=2.0,
                        param_groups=[{'params': [m.b], 'weight_decay': 0.0, 'lr_scale': 0.1}])
    assert [[id(p) for p in g['params']] for g in opt.param_groups] == [[id(m.b)], [id(m.w)]]
    g0, g1 = opt.param_groups
    assert (g0['weight_decay'], g0['lr'], g0['lr_scale'], g0['betas'], g0['eps']) == (0.0, 1e-3 * 0.1, 0.1, (0.8, 0.9), 1e-8)
    assert (g1['weight_decay'], g1['lr'], g1['lr_scale'], g1['betas']) == (0.3, 1e-3, 1.0, (0.8, 0.9))
    assert [p is q for p, q in zip(opt.arena.params, [m.w, m.b])] == [True, True]          # arena order = model.parameters() order
    sd = opt.state_dict()
    assert [g['lr_scale'] for g in sd['param_groups']] == [0.1, 1.0] and all('params' not in g for g in sd['param_groups'])
    m2 = _Tiny()                                        # every group's hyper-parameters travel with load_state_dict, lr_scale included
    opt3 = tu.FusedAdamW(m2, lr=5.0, param_groups=[{'params': [m2.b]}])
    opt3.load_state_dict(sd)
    assert [(g['lr'], g['lr_scale'], g['weight_decay'], tuple(g['betas'])) for g in opt3.param_groups] == [
        (1e-3 * 0.1, 0.1, 0.0, (0.8, 0.9)), (1e-3, 1.0, 0.3, (0.8, 0.9))]
    # no groups, no norm clip: the optimizer as it always was
    plain = tu.FusedAdamW(_Tiny(), lr=1e-3, weight_decay=1e-2, grad_clip=1.0)
    assert len(plain.param_groups) == 1 and set(plain.param_groups[0]) == {'params', 'lr', 'weight_decay', 'betas', 'eps'}
    assert plain.last_grad_norm is None


def test_train_config_and_lr_scale_defaults():
    from frankenstein_amd.utils import train_utils as tu
    assert tu.TrainConfig().grad_clip_norm == 0.0 and tu.TrainConfig().grad_clip == 1.0


def _cpu_gpt(bias):
    from frankenstein_amd.models import gpt2_model as g2
    return g2.GPT(g2.GPTConfig(block_size=64, vocab_size=211, n_layer=2, n_head=4, n_embd=64, dropout=0.0, bias=bias))


@pytest.mark.parametrize("bias", [True, False])
def test_decay_groups_reproduce_the_reference_split(bias):
    from frankenstein_amd.utils import train_utils as tu
    g = _cpu_gpt(bias)
    decay, nodecay = tu.decay_groups(g, 0.1)
    assert decay['weight_decay'] == 0.1 and nodecay['weight_decay'] == 0.0
    # the reference's rule over named_parameters() (which yields a tied tensor once): models/gpt2_model.py:288-298
    named = {n: p for n, p in g.named_parameters() if p.requires_grad}
    ref_decay = [p for p in named.values() if p.dim() >= 2]
    ref_nodecay = [p for p in named.values() if p.dim() < 2]
    assert [id(p) for p in decay['params']] == [id(p) for p in ref_decay]
    assert [id(p) for p in nodecay['params']] == [id(p) for p in ref_nodecay]
    # wte (tied to lm_head), wpe, and per layer c_attn, c_proj, c_fc, c_proj; per layer two LayerNorms (+ 4 biases), and ln_f
    L = 2
    assert len(decay['params']) == 2 + 4 * L
    assert len(nodecay['params']) == ((2 * L + 1) * 2 + 4 * L if bias else 2 * L + 1)
    assert sum(p is g.lm_head.weight for p in decay['params']) == 1 and g.transformer.wte.weight is g.lm_head.weight
    assert sum(p.numel() for p in decay['params']) + sum(p.numel() for p in nodecay['params']) == sum(p.numel() for p in g.parameters())


def test_configure_optimizers_on_the_cpu_is_torch_adamw():
    g = _cpu_gpt(True)
    for device_type in ("cpu", "cuda"):                  # 'cuda' with the parameters on the host: nothing for the arena kernels to run on
        opt = g.configure_optimizers(0.1, 3e-4, (0.9, 0.95), device_type)
        assert type(opt) is torch.optim.AdamW and len(opt.param_groups) == 2
        assert [pg['weight_decay'] for pg in opt.param_groups] == [0.1, 0.0]
        assert all(pg['lr'] == 3e-4 and tuple(pg['betas']) == (0.9, 0.95) for pg in opt.param_groups)
        assert sum(p is g.lm_head.weight for pg in opt.param_groups for p in pg['params']) == 1
