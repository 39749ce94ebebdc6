"""What hipcc compiled ctc_beam_kernel into (CPU suite: hipcc cross-compiles gfx950 without a GPU), from the compiler's resource remarks
alone.  The lexicon search is a third instantiation of the kernel; the plain and the n-gram instantiations are not to notice it.  They are
held to the resources they had before it existed (plain: 178 VGPRs, 10000 bytes of LDS; n-gram: 256 VGPRs + 1 AGPR, 19344 bytes; no scratch),
so that a change to the shared steps that moves them shows here and not in a timing.  The lexicon instantiations: no scratch, no VGPR spill."""
import pytest

from tools import kernel_resources as KR


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    _, remarks = KR.compile_isa("ctc.hip", tmp_path_factory.mktemp("isa"))
    return {n: r for n, r in KR.parse_remarks(remarks).items() if "ctc_beam_kernel" in n}


def test_existing_instantiations_keep_their_resources(table):
    plain = [r for n, r in table.items() if "Lb0ELb0E" in n]
    fused = [r for n, r in table.items() if "Lb1ELb0E" in n]
    assert len(plain) == 2 and len(fused) == 2, sorted(table)                 # {fp32, bf16} each
    for r in plain:
        assert (r["VGPRs"], r.get("AGPRs", 0), r["LDS Size"], r["ScratchSize"], r["VGPRs Spill"]) == (178, 0, 10000, 0, 0), r
    for r in fused:
        assert (r["VGPRs"], r.get("AGPRs", 0), r["LDS Size"], r["ScratchSize"], r["VGPRs Spill"]) == (256, 1, 19344, 0, 0), r


def test_lexicon_instantiations_have_no_scratch_and_no_spill(table):
    lex = {n: r for n, r in table.items() if "Lb1ELb1E" in n}
    assert len(lex) == 2 and len(table) == 6, sorted(table)                   # {fp32, bf16}; nothing else is instantiated
    for n, r in lex.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (n, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256 and r["LDS Size"] <= 32 * 1024, (n, r)   # one workgroup's registers; two workgroups' LDS a CU
