"""What hipcc compiled csrc/editdist.hip into (CPU suite: hipcc cross-compiles gfx950 without a GPU): the DP rows and the tokens of the
lanes' sequence are register arrays (up to 16 rows per lane), which only stay registers while every index is a compile-time constant.  A
change that makes one of them runtime-indexed would move them to scratch memory and only show as a slow kernel; this holds every kernel of
the file to no scratch and to the eight waves per SIMD that hide the one cross-lane move per anti-diagonal."""
import pytest

from tools import kernel_resources as KR


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    _, remarks = KR.compile_isa("editdist.hip", tmp_path_factory.mktemp("isa"))
    return KR.parse_remarks(remarks)


def test_no_scratch_and_full_occupancy(table):
    names = [n for n in table if "edit_distance_kernel" in n or "nbest_pairwise_kernel" in n or "mbr_rank_kernel" in n or "mwer_combine_kernel" in n]
    assert len(names) == 6 + 3 + 2, sorted(table)                       # three routes x {a, b on the lanes}, three pairwise routes
    for n in names:
        r = table[n]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)
        assert r["VGPRs"] <= 64 and r["Occupancy"] == 8, (n, r)
