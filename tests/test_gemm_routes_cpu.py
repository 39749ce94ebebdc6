"""The routing table of fk_gemm_nt / fk_gemm_tn, pinned through the host-side queries (kernels.gemm_nt_route / gemm_tn_route: no launch,
no GPU).  tests/test_gemm_routes_gpu.py runs the shapes of tests/cases.py on the kernels these tests say they reach; a changed threshold
fails here first instead of silently turning a GPU test into a second copy of another one."""
import pytest
import torch

from tests import cases

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def K():
    from frankenstein_amd import build
    build.build(verbose=False)
    from frankenstein_amd import kernels
    return kernels


@pytest.fixture(autouse=True)
def default_threshold(monkeypatch):
    monkeypatch.delenv("FK_NT_RING_MIN_TILES", raising=False)


def name(K, M, N, Kd, dtype=BF, vec_epi=True, mode=0, has_rope=False):
    return K.NT_ROUTE_NAMES[K.gemm_nt_route(M, N, Kd, dtype, vec_epi, mode, has_rope)]


def case_route(K, monkeypatch, route, M, N, Kd, ring_min, mode=0, has_rope=False):
    if ring_min is not None:
        monkeypatch.setenv("FK_NT_RING_MIN_TILES", ring_min)
    return name(K, M, N, Kd, F32 if route == "F32" else BF, N % 8 == 0, mode, has_rope)


def want(route):
    return "NT_STAGED_F32" if route == "F32" else route


def test_route_constants_match_the_header(K):
    import re
    from pathlib import Path
    hdr = (Path(__file__).resolve().parents[1] / "include" / "franken_hip.h").read_text()
    enum = re.search(r"enum \{ (FK_NT_RING2[^}]*) \};", hdr).group(1)
    vals = {k.strip()[3:]: int(v) for k, v in (e.split("=") for e in enum.split(","))}
    assert vals == {n: v for v, n in K.NT_ROUTE_NAMES.items() if v >= 0}
    assert int(re.search(r"#define FK_NT_ROUTE_F32 \((-?\d+)\)", hdr).group(1)) == K.NT_ROUTE_F32 < 0
    assert sorted(vals.values()) == list(range(8)) and vals["NT_LANE"] == 7      # NT_LANE: fk_gemm_nt_rope_route / fk_gemm_nt_swiglu_route only


@pytest.mark.parametrize("case", cases.NT_PLAIN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_plain_cases_reach_the_route_they_name(K, monkeypatch, case):
    route, M, N, Kd, ring_min = case
    assert case_route(K, monkeypatch, route, M, N, Kd, ring_min) == want(route)
    assert M % 128 != 0 and M % 256 != 0, "every route gets a ragged last row tile"
    assert Kd <= 384 and (4096 <= M <= 8300 if route in ("NT_RING2", "NT_RING192", "NT_RING128", "NT_BIG") else M <= 3100)


@pytest.mark.parametrize("case", cases.NT_SWIGLU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_swiglu_forward_cases_reach_the_route_they_name(K, monkeypatch, case):
    route, M, H, Kd, ring_min = case
    assert case_route(K, monkeypatch, route, M, 2 * H, Kd, ring_min, mode=1) == want(route)


@pytest.mark.parametrize("case", cases.NT_DSWIGLU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_swiglu_backward_cases_reach_the_route_they_name(K, monkeypatch, case):
    route, M, H, Kd, ring_min = case
    assert case_route(K, monkeypatch, route, M, H, Kd, ring_min, mode=2) == want(route)


@pytest.mark.parametrize("case", cases.NT_ROPE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_rope_cases_reach_the_route_they_name(K, monkeypatch, case):
    route, B, T, N, Kd, D, rot, off, qc, bias, per_sample, ring_min = case
    assert case_route(K, monkeypatch, route, B * T, N, Kd, ring_min, has_rope=True) == want(route)
    assert D % 8 == 0 and rot % D == 0 and rot <= N and qc % 8 == 0 and qc <= rot


def test_the_fused_matrix_covers_every_route_that_accepts_it():
    fused = {"NT_RING2", "NT_RING128", "NT_BIG", "NT_GLDS", "NT_GLDS4", "NT_STAGED", "F32"}
    for lst in (cases.NT_SWIGLU_CASES, cases.NT_DSWIGLU_CASES, cases.NT_ROPE_CASES):
        assert {c[0] for c in lst} == fused
    assert {c[0] for c in cases.NT_PLAIN_CASES} == fused | {"NT_RING192"}
    rope = cases.NT_ROPE_CASES
    assert {c[5] for c in rope} == {8, 16, 64, 128} and {c[2] for c in rope} == {5, 57, 300}
    for route in fused:                                     # per route: a shared and a per-sample table; rot_cols < N and == N somewhere
        assert {c[10] for c in rope if c[0] == route} == {True, False}, route
    assert any(c[6] == c[3] for c in rope) and any(c[6] < c[3] for c in rope) and any(c[7] > 0 for c in rope) and any(c[8] > 0 for c in rope)
    for route in ("NT_RING2", "NT_RING128"):                # short and odd T above one tile on the ring kernels
        assert {c[2] for c in rope if c[0] == route} == {5, 57, 300}, route


def test_row_threshold_4095_4096(K, monkeypatch):
    for N, big in ((256, "NT_BIG"), (512, "NT_BIG"), (384, "NT_GLDS4")):
        assert name(K, 4095, N, 64) == "NT_GLDS4"
        assert name(K, 4096, N, 64) == big                  # under the default threshold of 128 tiles no ring kernel
    monkeypatch.setenv("FK_NT_RING_MIN_TILES", "0")
    for N, ring in ((256, "NT_RING2"), (384, "NT_RING192"), (128, "NT_RING128"), (1152, "NT_RING2")):
        assert name(K, 4095, N, 64) in ("NT_GLDS4", "NT_GLDS")
        assert name(K, 4096, N, 64) == ring


def test_tile_count_256_257_between_the_two_double_buffered_kernels(K):
    assert name(K, 16 * 128, 16 * 128, 64) == "NT_GLDS4"                  # 256 tiles of 128 x 128
    assert name(K, 16 * 128 + 1, 16 * 128 - 128, 64) == "NT_GLDS4"        # 17 x 15 = 255
    assert name(K, 16 * 128 + 1, 16 * 128, 64) == "NT_GLDS"               # 17 x 16 = 272
    assert name(K, 257 * 128, 128, 64, vec_epi=False) == "NT_GLDS"        # 257 x 1
    assert name(K, 256 * 128, 128, 64, vec_epi=False) == "NT_GLDS4"


def test_default_ring_threshold_127_128_tiles_of_256(K, monkeypatch):
    assert name(K, 127 * 256, 256, 64) == "NT_BIG" and name(K, 127 * 256 + 1, 256, 64) == "NT_RING2"
    assert name(K, 31 * 256, 1024, 64) == "NT_BIG" and name(K, 31 * 256 + 1, 1024, 64) == "NT_RING2"          # 124 | 128
    assert name(K, 43 * 256, 384, 64) == "NT_GLDS" and name(K, 64 * 256, 384, 64) == "NT_RING192"            # 2 tile columns of 256: 86 | 128
    assert name(K, 63 * 256 + 1, 384, 64) == "NT_RING192" and name(K, 63 * 256, 384, 64) == "NT_GLDS"
    monkeypatch.setenv("FK_NT_RING_MIN_TILES", "127")
    assert name(K, 127 * 256, 256, 64) == "NT_RING2"                       # read per call


def test_column_classes_of_the_ring_kernels(K, monkeypatch):
    monkeypatch.setenv("FK_NT_RING_MIN_TILES", "0")
    M = 4200
    table = {128: "NT_RING128", 192: "NT_RING192", 256: "NT_RING2", 384: "NT_RING192", 512: "NT_RING2", 576: "NT_RING192", 640: "NT_RING128",
             768: "NT_RING2", 896: "NT_RING128", 960: "NT_GLDS", 1024: "NT_RING2", 1152: "NT_RING2", 1280: "NT_RING2", 1344: "NT_GLDS", 200: "NT_GLDS4"}
    for N, r in table.items():
        assert name(K, M, N, 64) == r, N
    # the 192-column tiles exist for the plain epilogue only: fused modes and RoPE take the 128-column ring
    # (N = 384), and where 128 does not divide N the 128 x 128 kernels
    for N, r in ((192, "NT_GLDS4"), (384, "NT_RING128"), (576, "NT_GLDS4")):
        assert name(K, M, N, 64, mode=1) == name(K, M, N, 64, mode=2) == name(K, M, N, 64, has_rope=True) == r, N
    for N in (256, 1152):
        assert name(K, M, N, 64, mode=1) == name(K, M, N, 64, mode=2) == name(K, M, N, 64, has_rope=True) == "NT_RING2", N


def test_scalar_epilogue_and_odd_k_keep_off_the_wide_kernels(K, monkeypatch):
    for ring_min in ("0", None):
        if ring_min is not None:
            monkeypatch.setenv("FK_NT_RING_MIN_TILES", ring_min)
        for N in (128, 256, 384, 1152):
            assert name(K, 8192, N, 64, vec_epi=False) in ("NT_GLDS4", "NT_GLDS")              # vec_epi = 0: no ring route, no NT_BIG
            assert name(K, 8192, N, 72) == "NT_STAGED" == name(K, 8192, N, 72, vec_epi=False)   # K % 64 != 0: register-staged
            assert name(K, 8192, N, 64, F32) == "NT_STAGED_F32"
    assert K.gemm_nt_route(8192, 256, 64, F32) == K.NT_ROUTE_F32 < 0


def test_route_query_refuses_nonsense(K):
    from frankenstein_amd import _lib
    with pytest.raises(_lib.FrankenHipError, match="bad problem"):
        K.gemm_nt_route(0, 128, 64)
    assert _lib.lib().fk_gemm_nt_route(128, 128, 64, 7, 1, 0, 0) == -1
    assert _lib.lib().fk_gemm_tn_route(128, 128, 64, 7, None, None) == -1
    assert _lib.lib().fk_gemm_tn_route(1000, 136, 72, _lib.FK_BF16, None, None) == 0     # both outputs are optional


@pytest.mark.parametrize("case", cases.TN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_tn_cases_and_their_splits(K, case):
    kernel, dt, M, N1, N2, nsplit, rps = case
    dtype = BF if dt == "bf16" else F32
    assert K.gemm_tn_route(M, N1, N2, dtype) == (kernel, nsplit, rps)
    assert nsplit * rps >= M
    from frankenstein_amd import _lib
    assert _lib.lib().fk_gemm_tn_workspace_bytes(M, N1, N2, K.fk_dtype(dtype)) == (nsplit * N1 * N2 * 4 if nsplit > 1 else 0)


def test_tn_cases_contain_empty_and_short_splits(K):
    """4163 x 904 x 1000 (bf16) and 2083 x 904 x 1000 (fp32): 16 splits, of which the last two start past M (all-zero slabs) and the
    last non-empty one has 3 rows; the issue's 4200 x 1024 x 1024 example behaves the same way."""
    for dtype, M in ((BF, 4163), (F32, 2083)):
        _, ns, rps = K.gemm_tn_route(M, 904, 1000, dtype)
        starts = [s * rps for s in range(ns)]
        assert [s >= M for s in starts].count(True) == 2 and starts[-2] >= M
        assert M - max(s for s in starts if s < M) == 3
        assert 904 % 128 != 0 and 1000 % 128 != 0
    _, ns, rps = K.gemm_tn_route(4200, 1024, 1024, BF)
    assert (ns, rps) == (16, 320) and 14 * rps >= 4200 > 13 * rps
    assert K.gemm_tn_route(16384, 2304, 384, BF)[0] == K.TN_BIG192 and K.gemm_tn_route(16384, 384, 128, BF)[0] == K.TN_BIG128
    assert K.gemm_tn_route(16383, 384, 128, BF)[0] == K.TN_SMALL == K.gemm_tn_route(16384, 384, 128, F32)[0]
