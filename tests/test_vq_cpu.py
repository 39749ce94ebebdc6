"""CPU-side checks of the vector-quantiser kernels (csrc/vq.hip): the host-only route predicate, argument validation before any launch,
the compiled kernels' resources, and the condition on the shared test inputs (tests/vq_ref.py) that the GPU tests' near-tie exclusion
rule rests on."""
import numpy as np
import pytest
import torch

from tests import vq_ref as VR


@pytest.fixture(scope="module")
def lib():
    from frankenstein_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_route_envelope(lib):
    from frankenstein_amd import _lib, kernels as K
    for D, Kc in ((16, 64), (64, 1024), (128, 1), (4, 7)):
        for dt in (_lib.FK_F32, _lib.FK_BF16):
            assert lib.fk_vq_route(D, Kc, dt) == _lib.VQ_FUSED, (D, Kc, dt)
        assert K.vq_route(D, Kc, torch.float32) and K.vq_route(D, Kc, torch.bfloat16)
    for D in (6, 132, 0):
        assert lib.fk_vq_route(D, 64, _lib.FK_F32) == _lib.VQ_CHAIN and not K.vq_route(D, 64, torch.bfloat16), D
    assert lib.fk_vq_route(64, 64, 7) == _lib.VQ_CHAIN and not K.vq_route(64, 64, torch.float16)
    assert lib.fk_vq_route(64, 0, _lib.FK_F32) == _lib.VQ_CHAIN and lib.fk_vq_route(64, 1 << 31, _lib.FK_F32) == _lib.VQ_CHAIN
    assert lib.fk_vq_route(64, (1 << 31) - 1, _lib.FK_F32) == _lib.VQ_FUSED


def test_argument_validation_comes_before_the_route(lib):
    """bad arguments are refused on the host with FK_EINVAL whether or not the shape is inside the envelope; a good call outside the
    envelope is FK_EUNSUPPORTED (the caller asks fk_vq_route first)"""
    from frankenstein_amd import _lib
    F = _lib.FK_F32
    assign = lambda x, ldx, D, dt=F, q=None, part=None, commit=None, ticket=None: lib.fk_vq_assign(
        x, ldx, 64, 64, q, None, 0, None, 0, part, commit, 0.0, ticket, 8, 8, D, dt, None)
    assert assign(64, 16, 16, dt=7) == -1 and b"dtype" in lib.fk_last_error()
    assert assign(None, 16, 16) == -1 and b"null" in lib.fk_last_error()
    assert assign(64, 8, 16) == -1 and b"bad shape" in lib.fk_last_error()                 # a row stride shorter than the row
    assert assign(64, 4, 6, dt=7) == -1 and b"dtype" in lib.fk_last_error()                # outside the envelope AND bad: EINVAL first
    assert assign(64, 8, 6) == -3 and b"envelope" in lib.fk_last_error()
    assert assign(64, 132, 132) == -3
    assert assign(64, 18, 16) == -1 and b"aligned" in lib.fk_last_error()
    assert assign(64, 16, 16, part=64) == -1 and b"go together" in lib.fk_last_error()     # partials without commit / ticket
    assert lib.fk_vq_bwd(64, None, None, None, 0.0, 64, 8, F, None) == -1
    assert lib.fk_vq_codebook_update(64, None, None, 64, 1, 64, 16, None, None, 8, 16, 0.8, 1e-5, 2.0, _lib.VQ_EMA, None) == -1 and b"EMA" in lib.fk_last_error()
    assert lib.fk_vq_codebook_update(64, None, None, 64, 1, 64, 8, None, None, 8, 16, 0.0, 0.0, 0.0, _lib.VQ_KMEANS, None) == -1   # ld_sums < D
    assert lib.fk_vq_codebook_update(64, None, None, 64, 1, 64, 16, None, None, 8, 16, 0.0, 0.0, 0.0, 5, None) == -1 and b"mode" in lib.fk_last_error()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("case", VR.LOOKUP_CASES)
def test_reference_inputs_have_no_near_ties(case, bf16):
    """the GPU test compares idx on every row whose float64 top-2 gap is >= 1e-5 and may exclude 1 % at the most: on these inputs the
    reference itself excludes (almost) none, from the fp32 values and from their bf16 roundings alike"""
    x, codes = VR.lookup_inputs(*case)
    if bf16:
        x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    _, gap, _, _ = VR.lookup(x, codes)
    assert (gap < VR.GAP).mean() <= 0.01, (case, float((gap < VR.GAP).mean()), float(gap.min()))


def test_planted_kmeans_data_is_well_separated():
    """the float64 Lloyd iteration on the planted data keeps a top-2 gap >= 1e-4 on every round, uses every cluster, and its mean best
    similarity does not decrease"""
    x, init, lab = VR.planted()
    xn, means, prev = VR.normalize(x), init.astype(np.float64), -1.0
    for _ in range(3):
        means, idx, counts, gap, score = VR.kmeans_round(xn, means)
        assert gap >= 1e-4 and counts.min() > 0 and score >= prev - 1e-12, (gap, counts, score, prev)
        prev = score
    assert counts.sum() == x.shape[0]


def test_reference_ema_matches_the_torch_chain():
    """vq_ref.ema restates the arithmetic of VectorQuantize._ema_update_chain (torch, fp32 on the CPU) without the re-seeding"""
    rng = np.random.default_rng(3)
    Kc, D, decay, eps = 33, 16, 0.8, 1e-5
    emb = VR.normalize(rng.standard_normal((Kc, D)))
    avg, cs = emb * 3.0, rng.uniform(2.5, 9.0, Kc)
    counts, sums = rng.integers(0, 9, Kc).astype(np.float64), rng.standard_normal((Kc, D))
    e1, a1, c1, dead = VR.ema(emb, avg, cs, counts, sums, decay, eps, 0.0)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32))
    tcs = t(cs).mul_(decay).add_(t(counts), alpha=1 - decay)
    tavg = t(avg).mul_(decay).add_(t(sums), alpha=1 - decay)
    n = tcs.sum()
    sm = (tcs + eps) / (n + Kc * eps) * n
    temb = torch.nn.functional.normalize(tavg / sm[:, None], dim=-1)
    assert not dead.any()
    np.testing.assert_allclose(c1, tcs.numpy(), atol=1e-5)
    np.testing.assert_allclose(a1, tavg.numpy(), atol=1e-5)
    np.testing.assert_allclose(e1, temb.numpy(), atol=1e-5)


def test_vq_assign_kernels_have_no_scratch(tmp_path):
    """the lookup keeps its B operand (up to 64 registers), one chunk of codes and 16 accumulators in registers at two waves per SIMD: a
    spill inside the chunk loop would only show as a slow tokenizer"""
    from tools import kernel_resources as KR
    table = KR.survey(tmp_path, sources=["vq.hip"])
    hits = {n: r for n, r in table.items() if "vq_assign_kernel" in n}
    assert len(hits) == 8, sorted(hits)                     # {fp32, bf16} x {16, 32, 64, 128}
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] + r.get("AGPRs", 0) <= 256 and r["Occupancy"] >= 2, (name, r)
        loops = KR.mfma_loops(r["_asm"], name)
        assert loops and max(l[3] for l in loops) == 0, (name, loops)


def test_lds_budget_is_a_static_assert():
    from frankenstein_amd import build as B
    assert "static_assert(VQ_LDS <= 160 * 1024" in (B.CSRC / "vq.hip").read_text()


def test_vector_quantize_records_kmeans_init():
    from frankenstein_amd.models import vq_brain as vq
    assert vq.VectorQuantize(16, 64, kmeans_init=True).kmeans_init is True and vq.VectorQuantize(16, 64).kmeans_init is False
    net = vq.SoundStream(C=32, D=16, codebook_size=64, n_electrodes=16)
    assert net.quantizer.kmeans_init is True and callable(net.init_codebook) and bool(net.quantizer._codebook.initted)


def test_planted_empty_cluster_stays_empty_in_the_reference():
    x, init, j = VR.planted_with_empty_cluster()
    xn, means = VR.normalize(x), init.astype(np.float64)
    for _ in range(2):
        means, idx, counts, gap, _ = VR.kmeans_round(xn, means)
        assert counts[j] == 0 and gap >= 1e-4 and counts.sum() == x.shape[0], (counts, gap)
    np.testing.assert_array_equal(means[j], init[j].astype(np.float64))
