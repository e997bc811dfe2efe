#!/usr/bin/env python3
"""tests/golden/act_paths.json -- one SHA-256 of the output bytes per case of tests/act_paths_cases.py (GroupNorm apply pass, every
convolution family's epilogue, the thin kernels, the elementwise kernel; every activation, with and without bias / residual / affine).

Needs an MI355X.  Run it on the build whose bits are to be pinned -- the PARENT of a change that must not move them -- and commit the
JSON; tests/test_gpu_act_paths.py replays the cases against it.  DCVIC_LIB_PATH selects the library as everywhere else.

    python tools/record_act_golden.py --commit <hash of the commit that was built> [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import act_paths_cases as A  # noqa: E402


def compiler_version() -> str:
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    try:
        out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
        return " | ".join(ln.strip() for ln in out.splitlines() if ln.startswith(("HIP version", "AMD clang version")))
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=A.GOLDEN)
    p.add_argument("--commit", required=True, help="full hash of the commit the library under DCVIC_LIB_PATH / in the tree was built from")
    a = p.parse_args()
    assert len(a.commit) == 40 and set(a.commit) <= set("0123456789abcdef"), "--commit takes the full 40-digit hash"
    import torch
    assert torch.cuda.is_available(), "record_act_golden.py needs a HIP device"
    hashes = A.record()
    A.GOLDEN = a.out
    A.write_golden(hashes, compiler_version(), a.commit)
    print(f"{len(hashes)} cases -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
