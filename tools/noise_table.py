#!/usr/bin/env python3
"""Writes the unit-normal half table of the sensor-noise stage into structuredetector_amd/csrc/sd_noise.hip.

    H[j] = round(1024 * Phi^-1((2048 + j + 0.5) / 4096)),  j = 0 .. 2047

with Phi^-1 = statistics.NormalDist().inv_cdf: the upper half of a 4096-level inverse-CDF table of the unit normal in Q10 (the lower half is
its mirror image, negated).  The values stand between the two marker lines of the source file; `python tools/noise_table.py` rewrites them in
place, `--check` only compares and exits 1 when the file is out of date, `--print` writes the block to stdout.  tests/noise_ref.py computes
the same table afresh and tests/test_noise_cpu.py compares it with what the library exports (`sd_noise_normal_table`).
"""
import argparse
import sys
from pathlib import Path
from statistics import NormalDist

SOURCE = Path(__file__).resolve().parent.parent / "structuredetector_amd" / "csrc" / "sd_noise.hip"
BEGIN = "// ---- begin generated: tools/noise_table.py ----"
END = "// ---- end generated ----"
PER_LINE = 16


def half_table():
    inv = NormalDist().inv_cdf
    return [int(round(1024.0 * inv((2048 + j + 0.5) / 4096.0))) for j in range(2048)]


def block():
    h = half_table()
    assert h[0] == 0 and h[-1] == 3756 and all(a <= b for a, b in zip(h, h[1:])), "the half table is not what the definition pins"
    lines = [BEGIN, "#define SD_NOISE_HALF_TABLE \\"]
    for at in range(0, len(h), PER_LINE):
        row = ", ".join(f"{v:4d}" for v in h[at:at + PER_LINE])
        lines.append(f"    {row}" + (", \\" if at + PER_LINE < len(h) else ""))
    lines.append(END)
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare only; exit 1 when the source file is out of date")
    ap.add_argument("--print", action="store_true", dest="show", help="write the block to stdout and leave the source file alone")
    a = ap.parse_args()
    new = block()
    if a.show:
        print(new)
        return 0
    text = SOURCE.read_text()
    i, j = text.index(BEGIN), text.index(END) + len(END)
    if text[i:j] == new:
        print(f"{SOURCE.name}: the half table is up to date")
        return 0
    if a.check:
        print(f"{SOURCE.name}: the half table is out of date (run tools/noise_table.py)", file=sys.stderr)
        return 1
    SOURCE.write_text(text[:i] + new + text[j:])
    print(f"{SOURCE.name}: half table rewritten")
    return 0


if __name__ == "__main__":
    sys.exit(main())
