"""The token-on-the-lane kernels of csrc/mlp_fused.hip without a GPU: which calls take them, and whether the inputs of
tests/test_lane_kernels_gpu.py can tell a wrong kernel from a right one.

  * The decision of fk_gemm_nt_swiglu / fk_gemm_nt_rope (fk_mlp_up_fused_ok / fk_qkv_rope_fused_ok, mu_grid_fills, pointer alignment,
    M > 0, pos_off >= 0) and of fk_mlp_bwd_fused between its two kernels is pinned through the host-side queries
    (kernels.gemm_nt_swiglu_route / gemm_nt_rope_route / mlp_bwd_fused_route): every row-count boundary on both sides, every clause of
    the predicates, each rejection falling back to the tiled route gemm_nt_route names.
  * Every case of tests/cases.py (LANE_*) reaches what its id names, and the matrix covers 1 .. 5 chunks, the row residues, every
    (rot_cols, q_cols) kind, both table kinds and both backward kernels.
  * On the float64 reference alone (tests/lane_ref.py), for every case:
      (a) a CPU model of the documented arithmetic — fp32 accumulation (exact on these operands), the fp32 epilogue in the kernels'
          evaluation order, bf16 rounding of what is stored — stays inside the bound of the GPU file.  Largest fractions of the bound:
          up g 0.9833, rope 0.9904, dh13 0.9833, dx 0.9855; saturated gates: g 0.9833 (the saturated units alone 0.9758), dh13 0.9762
          (the saturated units alone 0.9261), dx 0.9831 — all of it the bf16 rounding of the stored value (2^-8 |ref| is half an ulp
          just above a power of two).  Linear outputs of the model are bit-equal to the rounded reference.
      (b) every mix-up a lane kernel could commit moves at least one element of the reference past that bound (and changes the bits of
          a linear output): a dropped 16-wide k block of either product, the weights of chunk c +- 1, h1 and h3 swapped, the
          activations (or the h13 tile) of token m +- 1, 8, 32, 256, the rotation of position +- 1, of another sample, or the unscaled
          table on a query head, and an operand read (an output written) with another operand's leading dimension.
"""
import functools
import re
from pathlib import Path

import pytest
import torch

from tests import cases, lane_ref as LR
from tests.test_gemm_routes_gpu import check_bound

BF, F32 = torch.bfloat16, torch.float32
d = cases.LANE_D
SENTINEL = -7.0
WORST = {}


@pytest.fixture(scope="module")
def K():
    from frankenstein_amd import build
    build.build(verbose=False)
    from frankenstein_amd import kernels
    return kernels


@pytest.fixture(autouse=True)
def default_threshold(monkeypatch):
    monkeypatch.delenv("FK_NT_RING_MIN_TILES", raising=False)


def cid(c):
    return "-".join(str(x) for x in c)


def up(K, M, H, Kd=d, dtype=BF, align_ok=True, **ld):
    return K.NT_ROUTE_NAMES[K.gemm_nt_swiglu_route(M, H, Kd, align_ok=align_ok, dtype=dtype, **ld)]


def up_tiled(K, M, H, Kd=d, dtype=BF, vec_epi=True):
    return K.NT_ROUTE_NAMES[K.gemm_nt_route(M, 2 * H, Kd, dtype, vec_epi, 1, False)]


def qkv(K, M, N, T=1, D=64, rot=None, qc=0, Kd=d, dtype=BF, **kw):
    return K.NT_ROUTE_NAMES[K.gemm_nt_rope_route(M, N, Kd, T, D, N if rot is None else rot, qc, dtype=dtype, **kw)]


def qkv_tiled(K, M, N, Kd=d, dtype=BF, vec_epi=True):
    return K.NT_ROUTE_NAMES[K.gemm_nt_route(M, N, Kd, dtype, vec_epi, 0, True)]


def bwd(K, M, lddh):
    return K.MLP_BWD_ROUTE_NAMES[K.mlp_bwd_fused_route(M, lddh)]


# ----------------------------------------------------------------------------------------------- the predicate
def test_route_constants_match_the_header(K):
    hdr = (Path(__file__).resolve().parents[1] / "include" / "franken_hip.h").read_text()
    assert int(re.search(r"FK_NT_LANE = (\d+)", hdr).group(1)) == K.NT_LANE == 7 and K.NT_ROUTE_NAMES[K.NT_LANE] == "NT_LANE"
    m = re.search(r"enum \{ FK_MLP_BWD_HIPCC = (\d+), FK_MLP_BWD_ASM = (\d+) \};", hdr)
    assert (int(m.group(1)), int(m.group(2))) == (K.MLP_BWD_HIPCC, K.MLP_BWD_ASM) == (0, 1)
    assert K.MLP_BWD_ROUTE_NAMES == {0: "MLP_BWD_HIPCC", 1: "MLP_BWD_ASM"}


def test_row_count_boundaries_of_the_forward_kernels(K):
    """mu_grid_fills: 256-token workgroups that fill at least 70 % of their rounds of 256 — both sides of every boundary, for both
    entry points, the rejected side falling back to the tiled route"""
    assert cases.LANE_M_ACCEPTED == ((45825, 65536), (91649, 131072)) and cases.LANE_M_REJECTED == ((1, 45824), (65537, 91648), (131073, 137472))
    for lo, hi in cases.LANE_M_ACCEPTED + ((137473, 196608), (196609, 400000)):         # from three rounds on every count fills them
        for M in (lo, lo + 1, (lo + hi) // 2, hi):
            assert up(K, M, 64) == "NT_LANE" == qkv(K, M, 192), M
    for lo, hi in cases.LANE_M_REJECTED:
        for M in (lo, (lo + hi) // 2, hi - 1, hi):
            assert up(K, M, 64) == up_tiled(K, M, 64) != "NT_LANE", M
            assert qkv(K, M, 192) == qkv_tiled(K, M, 192) != "NT_LANE", M
    # the boundaries are whole workgroups: 179.2 per round -> 180 of 256, 358.4 -> 359 of 512, 537.6 -> 538 of 768
    assert [-(-m // 256) for m in (45825, 91649, 137473)] == [180, 359, 538]
    assert up(K, 4096, 128) == "NT_BIG" and up(K, 300, 64) == "NT_GLDS4"


def test_every_clause_of_the_up_projection_predicate(K):
    M, H = 45825, 64
    assert up(K, M, H) == "NT_LANE"
    assert up(K, M, H, Kd=320) == up_tiled(K, M, H, 320) and up(K, M, H, Kd=448) == up_tiled(K, M, H, 448)          # K != 384
    assert up(K, M, H, Kd=392) == up_tiled(K, M, H, 392) == "NT_STAGED"
    assert up(K, M, H, dtype=F32) == "NT_STAGED_F32"
    for Hbad in (48, 16, 100):                                                                                          # H % 32
        assert up(K, M, Hbad) == up_tiled(K, M, Hbad) != "NT_LANE", Hbad
    wide = dict(lda=d + 8, ldb=d + 16, ldh=2 * H + 24, ldg=H + 40)
    assert up(K, M, H, **wide) == "NT_LANE"
    for name, row in (("lda", d), ("ldb", d), ("ldh", 2 * H), ("ldg", H)):
        assert up(K, M, H, **{name: row}) == "NT_LANE"
        assert up(K, M, H, **{name: row + 4}) == up_tiled(K, M, H, vec_epi=name != "ldh") != "NT_LANE", name         # not a multiple of 8
        assert up(K, M, H, **{name: row - 8}) == up_tiled(K, M, H) != "NT_LANE", name                                  # shorter than its row
    assert up(K, M, H, ldb=2 ** 25 - 8) == "NT_LANE" and up(K, M, H, ldb=2 ** 25) == up_tiled(K, M, H)                  # 64 rows within 32 bits
    assert up(K, M, H, align_ok=False) == up_tiled(K, M, H, vec_epi=False) != "NT_LANE"                                # a misaligned pointer
    from frankenstein_amd import _lib
    assert _lib.lib().fk_gemm_nt_swiglu_route(0, H, d, d, d, 2 * H, H, 1, _lib.FK_BF16) == -1                          # M > 0
    assert _lib.lib().fk_gemm_nt_swiglu_route(M, H, d, d, d, 2 * H, H, 1, 7) == -1


def test_every_clause_of_the_qkv_predicate(K):
    M, N = 45825, 192
    tiled = qkv_tiled(K, M, N)
    assert tiled != "NT_LANE"
    for rot, qc in ((0, 0), (N, 0), (N, N), (128, 64)):
        assert qkv(K, M, N, rot=rot, qc=qc) == "NT_LANE"
    assert qkv(K, M, N, T=975, pos_off=5) == "NT_LANE" and qkv(K, M, N, T=3) == "NT_LANE"
    assert qkv(K, M, N, Kd=320) == qkv_tiled(K, M, N, 320) and qkv(K, M, N, Kd=392) == "NT_STAGED"                      # K != 384
    assert qkv(K, M, N, dtype=F32) == "NT_STAGED_F32"
    assert qkv(K, M, N, D=32) == tiled and qkv(K, M, N, D=128, rot=128) == tiled                                        # D != 64
    assert qkv(K, M, 96, rot=64) == qkv_tiled(K, M, 96) != "NT_LANE" and qkv(K, M, 200, rot=128) == qkv_tiled(K, M, 200) != "NT_LANE"     # N % 64
    assert qkv(K, M, N, has_bias=True) == tiled
    assert qkv(K, M, N, T=7) == tiled and 45825 % 7 != 0                                                               # M % T
    assert qkv(K, M, N, rot=32) == tiled and qkv(K, M, N, rot=128, qc=32) == tiled and qkv(K, M, N, rot=256) == tiled  # rot, q % 64; rot <= N
    assert qkv(K, M, N, pos_off=-1) == tiled and qkv(K, M, N, pos_off=0) == "NT_LANE"
    assert qkv(K, M, N, lda=d + 8, ldb=d + 16, ldc=N + 24) == "NT_LANE"
    for name, row in (("lda", d), ("ldb", d), ("ldc", N)):
        assert qkv(K, M, N, **{name: row + 4}) == qkv_tiled(K, M, N, vec_epi=name != "ldc") != "NT_LANE", name
        assert qkv(K, M, N, **{name: row - 8}) == tiled, name
    assert qkv(K, M, N, ldb=2 ** 25 - 8) == "NT_LANE" and qkv(K, M, N, ldb=2 ** 25) == tiled
    assert qkv(K, M, N, align_ok=False) == qkv_tiled(K, M, N, vec_epi=False) != "NT_LANE"
    from frankenstein_amd import _lib
    assert _lib.lib().fk_gemm_nt_rope_route(0, N, d, d, d, N, 0, 1, 0, 64, N, 0, 1, _lib.FK_BF16) == -1


def test_the_two_backward_kernels(K):
    for M in (128, 256, 1024, 393216):
        assert bwd(K, M, 3072) == "MLP_BWD_ASM", M
    for M in (1, 7, 127, 129, 255, 4133, 393253):
        assert bwd(K, M, 3072) == "MLP_BWD_HIPCC", M
    assert bwd(K, 128, 2 ** 24 - 8) == "MLP_BWD_ASM" and bwd(K, 128, 2 ** 24) == "MLP_BWD_HIPCC"          # M * lddh * 2 < 2^32
    assert bwd(K, 699008, 3072) == "MLP_BWD_ASM" and bwd(K, 699136, 3072) == "MLP_BWD_HIPCC" and 699136 % 128 == 0 == 699008 % 128
    assert 699008 * 3072 * 2 < 2 ** 32 <= 699136 * 3072 * 2
    from frankenstein_amd import _lib
    with pytest.raises(_lib.FrankenHipError, match="bad problem"):
        K.mlp_bwd_fused_route(0, 64)


# ----------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", cases.LANE_UP_CASES, ids=cid)
def test_up_cases_reach_the_route_they_name(K, case):
    route, M, H = case
    assert up(K, M, H) == route == "NT_LANE" and up(K, M, H, lda=d + 8) == route


@pytest.mark.parametrize("case", cases.LANE_QKV_CASES, ids=cid)
def test_qkv_cases_reach_the_route_they_name(K, case):
    route, B, T, N, rot, qc, off, per_sample = case
    assert qkv(K, B * T, N, T=T, rot=rot, qc=qc, pos_off=off, lda=d + 8) == route == "NT_LANE"


@pytest.mark.parametrize("case", cases.LANE_BWD_CASES, ids=cid)
def test_backward_cases_reach_the_kernel_they_name(K, case):
    kernel, M, H = case
    assert bwd(K, M, 2 * H) == kernel and M <= cases.LANE_BWD_ROWS


def test_padded_cases_reach_the_lane_kernels(K):
    M, H, (pa, pw, ph, pg) = cases.LANE_PAD_UP
    assert up(K, M, H, lda=d + pa, ldb=d + pw, ldh=2 * H + ph, ldg=H + pg) == "NT_LANE"
    assert len({d + pa, d + pw, 2 * H + ph, H + pg}) == 4
    B, T, N, rot, qc, off, per_sample, (pa, pw, po) = cases.LANE_PAD_QKV
    assert qkv(K, B * T, N, T=T, rot=rot, qc=qc, pos_off=off, lda=d + pa, ldb=d + pw, ldc=N + po) == "NT_LANE"
    assert len({d + pa, d + pw, N + po}) == 3
    assert sorted(bwd(K, M, 2 * H + pads[4]) for M, H, pads in cases.LANE_PAD_BWD) == ["MLP_BWD_ASM", "MLP_BWD_HIPCC"]
    for M, H, (py, p2, ph, p13, pdh, pdx) in cases.LANE_PAD_BWD:
        assert len({d + py, d + p2, 2 * H + ph, 2 * H + p13, 2 * H + pdh, d + pdx}) == 6
        assert {py, p2, ph, p13, pdh, pdx} == {8, 16, 24, 40, 56, 72}


def test_the_matrix_covers_chunks_rows_rotations_tables_and_both_backward_kernels():
    upc, qc, bc = cases.LANE_UP_CASES, cases.LANE_QKV_CASES, cases.LANE_BWD_CASES
    assert {H // 32 for _, _, H in upc} == {1, 2, 3, 5}
    for H in (32, 64, 96, 160):                             # per chunk count: one row in the last workgroup, whole workgroups, a cut store group
        rows = {M for _, M, h in upc if h == H}
        assert {45825, 46080, 49007} <= rows, H
    assert 45825 % 256 == 1 and 46080 % 256 == 0 and 49007 % 8 != 0 and 49007 % 16 != 0
    assert any(M >= 91649 for _, M, _ in upc) and ("NT_LANE", 91649, 32) in upc                 # two rounds, one chunk
    assert {c[3] // 64 for c in qc} == {1, 3, 6}
    for N in (64, 192, 384):
        kinds = {(rot, q) for _, _, _, n, rot, q, _, _ in qc if n == N}
        assert {(0, 0), (N, 0), (N, N)} <= kinds, N
        if N > 64:
            assert (2 * N // 3, N // 3) in kinds, N
    assert {(B, T) for _, B, T, *_ in qc} == {(45825, 1), (1, 45825), (47, 975), (15275, 3)}
    for bt in ((45825, 1), (1, 45825), (47, 975), (15275, 3)):
        assert {c[7] for c in qc if (c[1], c[2]) == bt} == {True, False}, bt                     # shared and per-sample tables
        assert {c[6] for c in qc if (c[1], c[2]) == bt} == {0, 5}, bt
    assert {H // 32 for _, _, H in bc} == {1, 2, 3, 4, 5}
    assert {M for _, M, _ in bc} >= {1, 7, 33, 127, 128, 129, 256, 393, 1000}
    for H in (32, 64, 96, 128, 160):
        assert {k for k, _, h in bc if h == H} == {"MLP_BWD_HIPCC", "MLP_BWD_ASM"}, H
    assert all(c in bc for c in cases.LANE_BWD_PAIR) and cases.LANE_BWD_PAIR[0][2] == cases.LANE_BWD_PAIR[1][2]
    assert any(M % 8 != 0 and M > 128 for _, M, _ in bc) and any(M < 8 for _, M, _ in bc)
    assert set(cases.LANE_SATURATED) == {8, 16, 32, 64, 88, 96, 128} and max(v for v in cases.LANE_SATURATED if v < 88.72) == 88


# ----------------------------------------------------------------------------------------------- conditions (a) and (b)
def record(tag, f):
    WORST[tag] = max(WORST.get(tag, 0.0), f)
    print(f"FRAC {tag} CPU_MODEL {f:.4f}")
    assert f <= 1.0, (tag, f)


def moved(what, mut, ref, mag, relf=2e-5):
    f = LR.frac(mut, ref, mag, relf)
    assert f > 1.0, f"{what}: the mutated reference stays inside the bound ({f:.3f})"


def bits_differ(what, mut, ref):
    assert not torch.equal(LR.bf16(mut), LR.bf16(ref)), f"{what}: the mutated linear output rounds to the same bits"


def shifts(M):
    return sorted({s % M for k in (1, 8, 32, 256) for s in (k, -k)} - {0})


def reread(t, ld_placed, ld_read):
    """t [R, C] laid out with leading dimension ld_placed in a sentinel-filled buffer, read back as [R, C] with ld_read: an operand
    read (ld_placed the true one) or an output written (ld_read the true one) with the wrong leading dimension"""
    R, C = t.shape
    flat = torch.full((R * max(ld_placed, ld_read) + C,), SENTINEL, dtype=t.dtype)
    flat.as_strided((R, C), (ld_placed, 1)).copy_(t)
    return flat.as_strided((R, C), (ld_read, 1)).clone()


def test_the_bound_is_the_projects(K):
    """LR.frac measures what check_bound asserts: the same verdict on a model inside the bound and on a mutation outside it"""
    a, w, acc, _ = LR.operands_cpu(300, 128, d, 1, LR.W_SCALE)
    g = LR.up_ref(acc)
    check_bound("swiglu_fwd", "CPU_MODEL", LR.up_model(acc)[1], g, g.abs(), BF)
    assert LR.frac(LR.up_model(acc)[1], g, g.abs()) <= 1.0 < LR.frac(g.roll(1, 0), g, g.abs())
    with pytest.raises(AssertionError, match="x its bound"):
        check_bound("swiglu_fwd", "MUTATED", g.roll(1, 0), g, g.abs(), BF)


def up_conditions(tag, a, w, acc, M, H, lds):
    g = LR.up_ref(acc)
    h_model, g_model = LR.up_model(acc)
    assert torch.equal(h_model, LR.bf16(acc))
    record(tag, LR.frac(g_model, g, g.abs()))

    def both(what, acc2):
        bits_differ(what + " (h13)", acc2, acc)
        moved(what + " (g)", LR.up_ref(acc2), g, g.abs())
    for kb in (0, 7, 23):
        both(f"k block {kb} dropped", acc - a[:, 16 * kb:16 * kb + 16].double() @ w[:, 16 * kb:16 * kb + 16].double().t())
    if H > 32:
        both("weights of chunk c + 1", acc.roll(-64, 1))
        both("weights of chunk c - 1", acc.roll(64, 1))
    a1, a3 = LR.split13(acc, M, H)
    both("h1 and h3 swapped", LR.join13(a3, a1))
    for s in shifts(M):
        both(f"activations of token m + {s}", acc.roll(-s, 0))
    lda, ldb, ldh, ldg = lds
    if lda != ldb:
        both("A read with ldb", reread(a, lda, ldb).double() @ w.double().t())
        both("W13 read with lda", a.double() @ reread(w, ldb, lda).double().t())
    both("A read with ldh", reread(a, lda, ldh).double() @ w.double().t())
    bits_differ("h13 written with lda", reread(acc, lda, ldh), acc)
    moved("g written with ldh", reread(g, ldh, ldg), g, g.abs())


@functools.lru_cache(maxsize=1)
def up_inputs(M, H):
    return LR.operands_cpu(M, 2 * H, d, LR.up_seed(M, H), LR.W_SCALE)


@pytest.mark.parametrize("case", cases.LANE_UP_CASES + [("NT_LANE-padded",) + cases.LANE_PAD_UP[:2]], ids=cid)
def test_up_projection_inputs_meet_both_conditions(case):
    _, M, H = case
    a, w, acc, _ = up_inputs(M, H)
    pads = cases.LANE_PAD_UP[2] if "padded" in case[0] else (0, 0, 0, 0)
    up_conditions("swiglu_fwd", a, w, acc, M, H, (d + pads[0], d + pads[1], 2 * H + pads[2], H + pads[3]))


def test_saturated_forward_inputs_meet_condition_a():
    M, H = 45825, 32
    a, w, acc, pre = LR.saturated_up_operands(M, H, cases.LANE_SATURATED)
    g = LR.up_ref(acc)
    h_model, g_model = LR.up_model(acc)
    assert torch.equal(h_model, LR.bf16(acc)) and bool(torch.isfinite(g_model).all())
    record("saturated_fwd", LR.frac(g_model, g, g.abs()))
    sat = [u for u, v in enumerate(pre) if abs(v) > 1]
    f_sat = LR.frac(g_model[:, sat], g[:, sat], g[:, sat].abs())
    print(f"FRAC saturated_fwd_units CPU_MODEL {f_sat:.4f}")
    a3 = LR.split13(acc, M, H)[1][:, sat]
    assert f_sat <= 1.0 and bool((a3 > 0).any()) and bool((a3 < 0).any()) and float(a3.abs().max()) >= 4 * float(a3.abs()[a3 != 0].min())


def qkv_inputs(case):
    _, B, T, N, rot, qc, off, per_sample = case[:8]
    M = B * T
    a, w, acc, g = LR.operands_cpu(M, N, d, LR.qkv_seed(M, N), LR.W_SCALE)
    return a, w, acc, LR.rope_tables(g, B, T, off, per_sample)


@pytest.mark.parametrize("case", cases.LANE_QKV_CASES + [("NT_LANE-padded",) + cases.LANE_PAD_QKV], ids=lambda c: cid(c[:8]))
def test_qkv_rope_inputs_meet_both_conditions(case):
    _, B, T, N, rot, qc, off, per_sample = case[:8]
    M = B * T
    a, w, acc, both = qkv_inputs(case)
    assert both.shape[-3] == off + T
    pairs = lambda **kw: LR.rope_pairs(both, B, T, N, rot, qc, off, per_sample, **kw)
    c, s = pairs() if rot else (None, None)
    ref, mag = LR.qkv_ref(acc, c, s, B, T, rot)
    model = LR.qkv_model(acc, c, s, B, T, rot)
    assert torch.equal(model[:, rot:], LR.bf16(acc[:, rot:]))
    if rot:
        record("rope", LR.frac(model[:, :rot], ref[:, :rot], mag[:, :rot]))

    def both_parts(what, acc2):
        r2, _ = LR.qkv_ref(acc2, c, s, B, T, rot)
        if rot:
            moved(what + " (rotated)", r2[:, :rot], ref[:, :rot], mag[:, :rot])
        if rot < N:
            bits_differ(what + " (linear)", r2[:, rot:], ref[:, rot:])
    for kb in (0, 23):
        both_parts(f"k block {kb} dropped", acc - a[:, 16 * kb:16 * kb + 16].double() @ w[:, 16 * kb:16 * kb + 16].double().t())
    if N > 64:
        both_parts("weights of chunk c + 1", acc.roll(-64, 1))
        both_parts("weights of chunk c - 1", acc.roll(64, 1))
    both_parts("the two tiles of a head swapped", acc.reshape(M, N // 64, 2, 32).flip(2).reshape(M, N))
    for sh in shifts(M):
        both_parts(f"activations of token m + {sh}", acc.roll(-sh, 0))
    if rot:
        rot_only = lambda what, **kw: moved(what, LR.qkv_ref(acc, *pairs(**kw), B, T, rot)[0][:, :rot], ref[:, :rot], mag[:, :rot])
        if off + T > 1:
            rot_only("position + 1", pos_shift=1)
            rot_only("position - 1", pos_shift=-1)
        if per_sample and B > 1:
            rot_only("another sample's row", sample_shift=1)
        if qc:
            rot_only("the unscaled table on a query head", unscaled_q=True)
    if len(case) > 8:
        pa, pw, po = case[8]
        both_parts("A read with ldb", reread(a, d + pa, d + pw).double() @ w.double().t())
        both_parts("W read with ldc", a.double() @ reread(w, d + pw, N + po).double().t())
        wrong = reread(ref, d + pa, N + po)
        moved("out written with lda (rotated)", wrong[:, :rot], ref[:, :rot], mag[:, :rot])
        bits_differ("out written with lda (linear)", wrong[:, rot:], ref[:, rot:])


@functools.lru_cache(maxsize=2)
def bwd_inputs(H):
    return LR.bwd_operands(H, cases.LANE_BWD_ROWS)


def bwd_conditions(tag, dy, w2t, dg, h13, w13t, M, H, lds=None):
    ref, mag = LR.bwd_ref(dg, h13)
    model = LR.bwd_model(dg, h13)
    assert bool(torch.isfinite(model).all())
    record(tag, LR.frac(model, ref, mag))
    xref, xmag, relf = LR.dx_ref(model, w13t)
    record(tag.replace("swiglu_bwd", "dx").replace("saturated_bwd", "saturated_dx"), LR.frac(LR.dx_model(model, w13t), xref, xmag, relf))
    if tag != "swiglu_bwd":
        return ref, mag, model
    dh = lambda what, dg2, h2=h13: moved(what + " (dh13)", LR.bwd_ref(dg2, h2)[0], ref, mag)
    dx = lambda what, x2: moved(what + " (dx)", x2, xref, xmag, relf)
    for kb in (0, 23):
        dh(f"k block {kb} of the first product dropped", dg - dy[:, 16 * kb:16 * kb + 16].double() @ w2t[:, 16 * kb:16 * kb + 16].double().t())
    for kb in (0, 2 * H // 16 - 1):
        dx(f"k block {kb} of the second product dropped", xref - model[:, 16 * kb:16 * kb + 16] @ w13t[:, 16 * kb:16 * kb + 16].double().t())
    if H > 32:
        for sh in (32, -32):
            dh(f"W2T of chunk c {sh:+d} rows", dg.roll(sh, 1))
            dh(f"the h13 tile of chunk c {sh:+d} units", dg, h13.roll(2 * sh, 1))
            dx(f"W13T of chunk c {sh:+d} units", model.roll(2 * sh, 1) @ w13t.double().t())
    a1, a3 = LR.split13(h13, M, H)
    dh("h1 and h3 swapped", dg, LR.join13(a3, a1))
    m1, m3 = LR.split13(model, M, H)
    dx("dh1 and dh3 swapped", LR.join13(m3, m1) @ w13t.double().t())
    for sh in shifts(M):
        dh(f"dy of token m + {sh}", dg.roll(-sh, 0))
        dh(f"the h13 tile of token m + {sh}", dg, h13.roll(-sh, 0))
        dx(f"dh13 of token m + {sh}", xref.roll(-sh, 0))
    if lds is not None and M > 1:
        ldy, l2, lh, l13, ldh, ldx = lds
        dh("dy read with ldw2t", reread(dy, ldy, l2).double() @ w2t.double().t())
        dh("W2T read with ldh", dy.double() @ reread(w2t, l2, lh).double().t())
        dh("h13 read with lddh", dg, reread(h13, lh, ldh))
        dx("W13T read with ldh", model @ reread(w13t, l13, lh).double().t())
        moved("dh13 written with ldh", reread(ref, lh, ldh), ref, mag)
        dx("dx written with lddy", reread(xref, ldy, ldx))
    return ref, mag, model


@pytest.mark.parametrize("case", cases.LANE_BWD_CASES + [("padded", M, H, pads) for M, H, pads in cases.LANE_PAD_BWD], ids=lambda c: cid(c[:3]))
def test_backward_chain_inputs_meet_both_conditions(case):
    _, M, H = case[:3]
    dy, w2t, dg, h13, w13t = (t[:M] if t.shape[0] == cases.LANE_BWD_ROWS else t for t in bwd_inputs(H))
    lds = (d, d, 2 * H, 2 * H, 2 * H, d)
    if len(case) > 3:
        py, p2, ph, p13, pdh, pdx = case[3]
        lds = (d + py, d + p2, 2 * H + ph, 2 * H + p13, 2 * H + pdh, d + pdx)
    bwd_conditions("swiglu_bwd", dy, w2t, dg, h13, w13t, M, H, lds if len(case) > 3 else None)


def test_saturated_backward_inputs_meet_condition_a():
    H, M = 32, 129
    dy, w2t, dg, h13, w13t, pre = LR.saturated_bwd_operands(H, M, cases.LANE_SATURATED)
    ref, mag, model = bwd_conditions("saturated_bwd", dy, w2t, dg, h13, w13t, M, H)
    cols = [8 * (u // 4) + u % 4 + o for u, v in enumerate(pre) if abs(v) > 1 for o in (0, 4)]
    f_sat = LR.frac(model[:, cols], ref[:, cols], mag[:, cols])
    print(f"FRAC saturated_bwd_units CPU_MODEL {f_sat:.4f}")
    assert f_sat <= 1.0
    a3 = LR.split13(h13, M, H)[1][:, :len(pre)]
    assert bool((a3 > 0).any()) and bool((a3 < 0).any()) and float(a3.abs().max()) >= 4 * float(a3.abs()[a3 != 0].min())
