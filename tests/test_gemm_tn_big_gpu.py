"""The large-tile weight-gradient kernel (csrc/gemm.hip, gemm_tn_big_kernel<128 | 192>) at the edges of its rotated stage loop, and the
SwiGLU-interleaved slab reduction (fk_gemm_tn_swiglu), bit for bit.

The loop reads a stage's first fragments during the stage before it, waits for the next stage in the middle of the current one and
requests the stage three ahead behind its MFMAs, so what can go wrong depends on the number of 32-row stages of a split: 0 (a split that
starts past M still writes its all-zero slab), 1, 2, 3 (fewer stages than ring slots), odd and even counts, and the last split being
shorter than the others.  The shapes are the smallest the large-tile route accepts (M >= 16 384); every case first asserts the split plan
it was chosen for (kernels.gemm_tn_route), then the stages of the last non-empty split and the number of empty splits that follow from it.

Method as tests/test_gemm_routes_gpu.py::test_gemm_tn_exact: small-integer operands with an asymmetric ramp in one column of each, A a
view with row stride N1 + 8, |ref| < 2^24 asserted, the result bit-equal to float64: plain, accumulate=True into a buffer of 3.0, an
out= view with ldc > N2 (neighbouring columns untouched), and the same launch a second time (torch.equal to the first)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (kernel, N1, N2, M, nsplit, rows_per_split, stages of the last non-empty split or "even", empty splits)
CASES = [
    (128, 384, 128, 16736, 32, 576, 1, 2),
    (128, 384, 128, 16768, 32, 576, 2, 2),
    (128, 384, 128, 16800, 32, 576, 3, 2),
    (128, 384, 128, 16864, 32, 576, 5, 2),
    (128, 384, 384, 16736, 32, 576, 1, 2),            # three column tiles
    (192, 384, 192, 16736, 32, 576, 1, 2),            # 128 does not divide N2: the 192-column tile
    (192, 384, 192, 16800, 32, 576, 3, 2),
    (192, 3072, 384, 16384, 16, 1024, "even", 0),     # N1 >= 2048 and N2 % 192 == 0: the 192-column tile, 16 tiles
    (192, 3072, 384, 16416, 16, 1088, 3, 0),
    (192, 3072, 384, 16480, 16, 1088, 5, 0),
]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from frankenstein_amd import kernels
    return kernels


def cid(c):
    return "-".join(str(x) for x in c)


def operands(M, N1, N2, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, N1 + 8), generator=g).float()
    b = torch.randint(-2, 3, (M, N2), generator=g).float()
    a[:, 3] += (torch.arange(M) % 5).float()
    b[:, 1] += (torch.arange(M) % 3).float()
    ref = a[:, :N1].double().t() @ b.double()
    assert float(ref.abs().max()) < 2 ** 24
    return a.to(BF).cuda()[:, :N1], b.to(BF).cuda(), ref.float()          # A with row stride N1 + 8


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_gemm_tn_big_exact(K, case):
    kernel, N1, N2, M, nsplit, rps, last_stages, empty = case
    assert K.gemm_tn_route(M, N1, N2, BF) == (kernel, nsplit, rps)
    full, rest = divmod(M, rps)
    assert nsplit - full - (1 if rest else 0) == empty
    stages = (rest if rest else rps) // 32
    assert (stages % 2 == 0 and stages >= 4) if last_stages == "even" else stages == last_stages
    ad, bd, ref = operands(M, N1, N2, M + N1)
    first = K.gemm_tn(ad, bd)
    assert torch.equal(first.cpu(), ref)
    assert torch.equal(K.gemm_tn(ad, bd), first)
    acc = torch.zeros(N1, N2, device="cuda")
    acc.fill_(3.0)
    K.gemm_tn(ad, bd, out=acc, accumulate=True)
    assert torch.equal(acc.cpu(), ref + 3)
    buf = torch.zeros(N1, N2 + 16, device="cuda")
    buf.fill_(3.0)
    K.gemm_tn(ad, bd, out=buf[:, 8:8 + N2])
    got = buf.cpu()
    assert torch.equal(got[:, 8:8 + N2], ref)
    assert bool((got[:, :8] == 3).all()) and bool((got[:, 8 + N2:] == 3).all())


def test_swiglu_interleaved_reduction_matches_temporary_plus_add2d(K):
    """fk_gemm_tn_swiglu adds the de-interleaved rows to both (pre-filled) gradients in the slab reduction: bit-equal to fk_gemm_tn into a
    temporary followed by the two add2d launches it replaces (engine.wgrad), computed here, and to float64 on these exact operands."""
    H, Kd, M = 384, 384, 16384
    assert K.gemm_tn_route(M, 2 * H, Kd, BF) == (128, 32, 512)
    ad, bd, ref = operands(M, 2 * H, Kd, 7)
    g = torch.Generator().manual_seed(11)
    fill = [torch.randint(-8, 9, (H, Kd), generator=g).float().cuda() for _ in range(2)]
    want = [f.clone() for f in fill]
    dw = K.gemm_tn(ad, bd)
    v = dw.view(H // 4, 8 * Kd)
    K.add2d_(want[0].view(H // 4, 4 * Kd), v[:, :4 * Kd])
    K.add2d_(want[1].view(H // 4, 4 * Kd), v[:, 4 * Kd:])
    got = [f.clone() for f in fill]
    assert K.gemm_tn_swiglu_ok(ad, bd, got[0], got[1])
    K.gemm_tn_swiglu_(ad, bd, got[0], got[1])
    r = ref.view(H // 4, 2, 4, Kd)
    for i in range(2):
        assert torch.equal(got[i], want[i])
        assert torch.equal(got[i].cpu(), fill[i].cpu() + r[:, i].reshape(H, Kd))
