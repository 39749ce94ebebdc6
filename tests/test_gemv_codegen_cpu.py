"""What hipcc made of the fk_gemv_nt kernels (tools/kernel_resources.py on csrc/gemv.hip with the build's own flags), and the host-side
argument checks of the entry point.  No GPU needed."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import kernel_resources as KR  # noqa: E402


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return KR.survey(tmp_path_factory.mktemp("isa_gemv"), ("gemv.hip",))


def test_every_gemv_kernel_is_scratch_free_at_two_waves_per_simd(table):
    """the accumulators (up to 16 rows x 4 columns per lane) and the weight pieces in flight stay in registers: no scratch, and at
    least two waves per SIMD (registers and the LDS activation chunk together) so that one wave's loads cover the other's arithmetic"""
    hits = {n: r for n, r in table.items() if "gemv" in n}
    assert len(hits) == 2 * 5 * 3, sorted(hits)                 # {fp32, bf16} x row bucket {1, 2, 4, 8, 16} x columns per wave {1, 2, 4}
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["Occupancy"] >= 2, (name, r)


def test_gemv_argument_validation_needs_no_gpu():
    """everything outside the envelope is refused on the host before any launch; M > 16 is not forwarded anywhere"""
    from frankenstein_amd import _lib, build
    build.build(verbose=False)
    lib, BF, F32 = _lib.lib(), _lib.FK_BF16, _lib.FK_F32
    call = lambda A=16, lda=64, W=32, ldw=64, C=48, ldc=64, M=2, N=64, K=64, res=None, ldr=0, gamma=None, beta=None, flags=0, dt=BF, odt=BF: \
        lib.fk_gemv_nt(A, lda, W, ldw, C, ldc, M, N, K, None, res, ldr, gamma, beta, 1e-5, flags, dt, odt, None)
    err = lambda: lib.fk_last_error()
    assert call(dt=7) == -1 and b"dtype" in err()
    assert call(dt=F32, odt=BF) == -1 and b"out_dtype" in err()
    for M in (0, 17, -1, 1 << 40):
        assert call(M=M) == -1 and b"outside 1..16" in err()
    assert call(N=0) == -1 and b"empty problem" in err()
    assert call(N=1 << 31) == -1 and b"int32" in err()
    assert call(K=12, lda=16, ldw=16) == -1 and b"multiple of 8" in err()
    assert call(K=6, lda=8, ldw=8, dt=F32, odt=F32) == -1 and b"multiple of 4" in err()
    assert call(A=None) == -1 and b"null" in err()
    assert call(lda=56) == -1 and b"leading dimensions" in err()
    assert call(ldw=56) == -1 and b"leading dimensions" in err()
    assert call(ldc=63) == -1 and b"leading dimensions" in err()
    assert call(res=64, ldr=63) == -1 and b"leading dimensions" in err()
    assert call(W=34) == -1 and b"16-byte aligned" in err()
    assert call(A=18) == -1 and b"16-byte aligned" in err()
    assert call(ldw=68) == -1 and b"16-byte aligned" in err()
    assert call(flags=2) == -1 and b"flags" in err()
    assert call(beta=64) == -1 and b"ln_beta" in err()
