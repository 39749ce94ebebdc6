"""The engine-level case table (tests/engine_cases.py) without a GPU: every case reaches the paths its id names, according to the host-side
queries engine.py's Functions ask themselves; every reachable path of every query is reached in every compute dtype that can reach it;
and the float64 reference of tests/engine_ref.py is sharp enough for the bound the GPU tests use — each planted bookkeeping defect moves
some checked tensor by at least twice the bound on every case it applies to, while the rounding model itself stays inside the bound."""
import pytest
import torch

from tests import engine_cases as EC
from tests import engine_ref as ER

IDS = [c.id for c in EC.CASES]

# query -> name -> the compute dtypes that can reach it
REACHABLE = {
    "proj": {"rope_ps": ("bf16",), "rope": EC.DTYPES, "ident_ps": ("bf16",), "plain": EC.DTYPES},
    "rope_bwd": {"fused": EC.DTYPES, None: EC.DTYPES},
    "mlp": {"swiglu_fused": EC.DTYPES, "swiglu": EC.DTYPES, "gelu": EC.DTYPES},
    "mlp_bwd": {"one_launch": ("bf16",), "dswiglu": EC.DTYPES, "plain": EC.DTYPES},
    "wgrad": {n: EC.DTYPES for n in ("tensors", "swiglu_slab", "swiglu_add", "adjacent", "split_add")},
    "norm_bwd": {"arena": EC.DTYPES, "tensors": EC.DTYPES},
}


@pytest.mark.parametrize("case", EC.CASES, ids=IDS)
def test_case_reaches_the_paths_it_names(case):
    assert ER.query_paths(case) == case.paths


def test_every_reachable_path_is_reached_in_every_dtype_that_can():
    seen = set()
    for c in EC.CASES:
        for q, v in c.paths.items():
            for name in (v.values() if isinstance(v, dict) else [v]):
                seen.add((q, name, c.dtype))
    missing = [(q, n, dt) for q, names in REACHABLE.items() for n, dts in names.items() for dt in dts if (q, n, dt) not in seen]
    assert not missing, missing
    stray = {(q, n, dt) for q, n, dt in seen if dt not in REACHABLE[q].get(n, ())}
    assert not stray, stray
    # the two arms entered as unreachable are the ones REACHABLE leaves out, and the queries still name them
    from frankenstein_amd import engine as E
    assert {(q, n) for q, n, _ in EC.UNREACHABLE} == {("attn_proj_path", "plain_rope"), ("attn_bwd_rope_path", "kernel")}
    assert E.attn_proj_path(2, 72, 2, 12, True, 0, False) == "plain_rope" and E.attn_bwd_rope_path(True, 6) == "kernel"
    for D in (8, 16, 32, 64, 128):          # every head_dim the attention kernels accept takes the fused arms
        for H in (1, 2, 3, 4):
            assert E.attn_proj_path(2, 72, H, D, True, 0, False) in ("rope", "rope_ps") and E.attn_bwd_rope_path(True, D) == "fused"


def test_every_in_place_arena_case_has_a_side_stream_twin():
    arena = [c for c in EC.CASES if c.arena is not None]
    inplace = {(c.fn, c.name, c.dtype) for c in arena if ER.arena_params(c) and c.name != "arena_one_outside"}
    assert inplace == {(c.fn, c.name, c.dtype) for c in arena if c.stream}


def test_slab_rows_is_the_smallest_row_count_with_a_split_plan():
    from frankenstein_amd import kernels as K
    assert K.gemm_tn_route(EC.SLAB_ROWS, 128, 128, torch.bfloat16)[1] > 1
    assert all(K.gemm_tn_route(M, 128, 128, torch.bfloat16)[1] == 1 for M in range(1, EC.SLAB_ROWS))


def test_one_launch_rows_is_the_smallest_ragged_count():
    (c,) = [c for c in EC.CASES if c.name == "one_launch"]
    rows = c.kw["B"] * c.kw["N"]
    assert rows == 32769 and rows % 128 != 0 and c.kw["d"] == 384 and c.kw["hidden"] == 32


def test_g0_is_small_dyadic_and_nonzero():
    g0 = ER.g0_pattern(1000).double()
    assert bool((g0 != 0).all()) and bool(((g0 * 2) == (g0 * 2).round()).all()) and float(g0.abs().max()) <= 4.0


@pytest.mark.parametrize("case", EC.CASES, ids=IDS)
def test_rounding_model_stays_inside_the_bound(case):
    """by construction in bf16 (MARGIN times its own largest relative error); a statement about the fp32 bound in fp32 mode"""
    inp, ref, model, bnd = ER.case_data(case)
    for n in ref:
        assert torch.isfinite(ref[n]).all() and torch.isfinite(model[n]).all(), n
        assert bool(((model[n] - ref[n]).abs() <= bnd[n]).all()), (n, float(((model[n] - ref[n]).abs() - bnd[n]).max()))


def _moved(case, defect, inp, ref, bnd):
    """largest |defective - ref| / bound over the checked tensors"""
    worst = 0.0
    if defect in ("arena_write", "arena_twice"):
        lay, total = ER.arena_layout(case, inp)
        g0 = ER.g0_pattern(total).double()
        for n in ER.arena_params(case):
            r = ref["d" + n]
            # the arena check compares grad - g0 with ref: written instead of added leaves ref - g0 there, added twice 2 ref
            delta = g0[lay[n][0]:lay[n][0] + lay[n][1]].view(r.shape) if defect == "arena_write" else r
            worst = max(worst, float((delta.abs() / bnd["d" + n].clamp_min(1e-300)).max()))
        return worst
    bad = ER.reference(case, inp, defect=defect)
    for n in ref:
        d = (bad[n] - ref[n]).abs()
        if float(d.max()) > 0:
            worst = max(worst, float((d / bnd[n].clamp_min(1e-300)).max()))
    return worst


@pytest.mark.parametrize("case", [c for c in EC.CASES if not c.stream], ids=[c.id for c in EC.CASES if not c.stream])
def test_every_planted_defect_moves_a_checked_tensor_by_twice_the_bound(case):
    inp, ref, model, bnd = ER.case_data(case)
    for defect in ER.defects_for(case):
        moved = _moved(case, defect, inp, ref, bnd)
        print(f"DEFECT {case.id} {defect} moved {moved:.3g} x bound")
        assert moved >= 2.0, (defect, moved)


def test_every_listed_defect_is_planted_somewhere():
    seen = {d if isinstance(d, str) else d[0] for c in EC.CASES for d in ER.defects_for(c)}
    assert seen == set(ER.ALL_DEFECTS)
    sums = {d[1] for c in EC.CASES for d in ER.defects_for(c) if not isinstance(d, str)}
    assert sums >= {"pb", "qkv_b", "up_b", "down_b", "ln_w", "ln_b", "space", "mask_token", "emb_b", "b"}
