"""What hipcc compiled csrc/lora.hip into (CPU suite: hipcc cross-compiles gfx950 without a GPU), from the compiler's resource remarks
alone.  fk_lora_fwd keeps one or two 32 x 32 accumulator tiles, their operand form and an output tile in registers, and the weight-gradient
kernel 64 accumulators per lane; every index into them is a compile-time constant.  A change that makes one runtime-indexed would move
them to scratch memory and only show as a slow kernel.  Declared budget: no scratch, no spills; the forward within 168 registers (three
waves per SIMD, two workgroups per CU for the r <= 32 form), the weight gradient within 96 (five waves), merge and reduce within 32."""
import pytest

from tools import kernel_resources as KR


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    _, remarks = KR.compile_isa("lora.hip", tmp_path_factory.mktemp("isa"))
    return KR.parse_remarks(remarks)


def test_no_scratch_and_declared_registers(table):
    budget = {"lora_fwd_kernel": (4, 168, 3), "lora_wgrad_kernel": (2, 96, 5), "lora_wgrad_reduce_kernel": (1, 32, 8), "lora_merge_kernel": (2, 32, 8)}
    seen = {k: 0 for k in budget}
    for n, r in table.items():
        kind = next((k for k in sorted(budget, key=len, reverse=True) if k in n), None)
        assert kind is not None, n
        seen[kind] += 1
        count, vgprs, waves = budget[kind]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= vgprs and r["Occupancy"] >= waves, (n, r)
    assert seen == {k: v[0] for k, v in budget.items()}, seen            # {bf16, fp32} x {r <= 32, r <= 64}; {bf16, fp32}; one; {bf16, fp32}
