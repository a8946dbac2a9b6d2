#!/usr/bin/env python3
"""Writes tests/golden/mfb_pack/<case>.bin for tests/test_gpu_mfb_pack.py::test_packed_backsub_golden_bytes: the step of the first matrix-free LM trial of each golden case
and the scalars its finishing workgroup publishes, raw float64.  Run ONCE on the GPU with the library of the commit before the back-substitution packed its single-batch
supernodes (NLLS_AMD_LIB=/path/to/that/libnlls_amd.so python tools/mfb_pack_golden.py [outdir]); the test then holds every later library to these bytes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["NLLS_SUPERNODE_PIECE"] = "128"

import numpy as np

from tests import test_gpu_mfb_pack as T


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    for nbig, ntiny in T.GOLDEN_CASES:
        x, sc = T.golden_trial(nbig, ntiny)
        np.concatenate([x, sc]).astype(np.float64).tofile(os.path.join(out, T.golden_name(nbig, ntiny) + ".bin"))
        print(f"{T.golden_name(nbig, ntiny)}: {x.size} step entries + {sc.size} scalars, cost {sc[0]!r}")


if __name__ == "__main__":
    main()
