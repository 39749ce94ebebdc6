"""Did a source-level change reach the device code?  Compiles every source of this tree and of a checkout of the parent commit
device-only with the build's own flags and compares the assembly, the `__hip_cuid_<hex>` symbol (a hash of the source text) masked.
Per source: `identical`, or the kernels whose bodies differ with their instruction counts and resource figures, parent -> this tree.
Local labels and loop comments carry the ordinal of their function (BB<n>_<m>), so a source whose kernels are merely emitted in another order (the order
of first instantiation on the host side) differs as a file and not in any body: that is reported as such.

    python tools/device_asm_diff.py PARENT_TREE [SRC...]       # PARENT_TREE: a git worktree or an export of the parent commit
"""
from __future__ import annotations

import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

from kernel_resources import ROOT, compile_isa, parse_remarks

FIGURES = ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "VGPRs Spill", "SGPRs Spill", "Occupancy")


def functions(asm: str) -> dict:
    """symbol -> its lines from the label to .Lfunc_end, the function's ordinal in local labels masked (and the padding between a label
    and its loop comment, which depends on the ordinal's width)"""
    names = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M))
    out, cur = {}, None
    for line in re.sub(r"(?m)^(\.LBB_\d+:) +;", r"\1 ;", re.sub(r"BB\d+_", "BB_", asm)).splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur.append(line)
    return out


def n_instr(body) -> int:
    return sum(bool(re.match(r"\s+[a-z]\w*(\s|$)", l)) for l in body)


def diff_source(src: str, parent: Path, tmp: Path) -> str:
    sides = []
    for name, root in (("parent", parent), ("new", ROOT)):
        (tmp / name).mkdir(exist_ok=True)
        asm, remarks = compile_isa(src, tmp / name, root)
        sides.append((re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", asm.read_text()), parse_remarks(remarks)))
    (a, ra), (b, rb) = sides
    if a == b:
        return f"{src}: identical"
    fa, fb = functions(a), functions(b)
    lines = [f"{src}: differs"]
    for k in sorted(set(fa) | set(fb)):
        if fa.get(k) != fb.get(k):
            lines.append(f"  {k}\n    instructions {n_instr(fa.get(k, []))} -> {n_instr(fb.get(k, []))}   " +
                         "  ".join(f"{f} {ra.get(k, {}).get(f)} -> {rb.get(k, {}).get(f)}" for f in FIGURES))
    if len(lines) == 1:
        return f"{src}: identical function bodies ({len(fa)}), emitted in another order"
    return "\n".join(lines)


if __name__ == "__main__":
    from frankenstein_amd import build as B
    parent, sources = Path(sys.argv[1]).resolve(), sys.argv[2:] or B.SOURCES
    tmp = Path(tempfile.mkdtemp())
    with ThreadPoolExecutor(max_workers=6) as ex:
        for text in ex.map(lambda s: diff_source(s, parent, tmp), sources):
            print(text, flush=True)
