"""Registers, scratch, occupancy and LDS of kernels from a gfx950 cross-compile (no device).

    python tools/kernel_resources.py [PATTERN]

compiles madpose_amd/csrc/kernels/kernels.hip with -Rpass-analysis=kernel-resource-usage
into a temporary directory and prints one line per kernel whose demangled name matches
PATTERN (a regular expression; default: the multi-pair solve stages of hypothesize_batch.h
and their single-pair counterparts).  profiles/hypothesize_batch/resource_usage.txt is this
tool's output.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madpose_amd.build import CSRC, FLAGS, HIPCC  # noqa: E402

DEFAULT = (r"hyp_|md_exact_kernel<\d, [24]>|pt_roots5_group_kernel|pt_pencil6|pt_roots7|pt_tail\d_group_kernel"
           r"|pt_compact")
FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), (r"ScratchSize \[bytes/lane\]", "scratch"),
          (r"Occupancy \[waves/SIMD\]", "occupancy"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"),
          (r"LDS Size \[bytes/block\]", "lds")]


def main():
    pattern = re.compile(sys.argv[1] if len(sys.argv) > 1 else DEFAULT)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [HIPCC, "-x", "hip"] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                              os.path.join(CSRC, "kernels", "kernels.hip"), "-o",
                                              os.path.join(tmp, "kernels.o")]
        log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    report(log, pattern)


def report(log, pattern):
    blocks = re.split(r"remark: [^\n]*Function Name: ", log)[1:]
    names = [b.split(" ", 1)[0] for b in blocks]
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    rows = {}
    for name, block in zip(plain.split("\n"), blocks):
        short = re.sub(r"\(.*", "", name.replace("mp::(anonymous namespace)::", "")).replace("void ", "")
        if not pattern.search(short):
            continue
        vals = []
        for key, label in FIELDS:
            m = re.search(key + r": (\d+)", block)
            vals.append(f"{label} {m.group(1) if m else '?':>4}")
        rows[short] = "  ".join(vals)
    print("# gfx950 cross-compile (-O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage); scratch in "
          "bytes per lane")
    for short in sorted(rows):
        print(f"{short:34s} {rows[short]}")


if __name__ == "__main__":
    main()
