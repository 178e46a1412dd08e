#!/usr/bin/env python3
"""Record tests/golden/rollout_prologue.npz: the bytes of the rollout kernel's costs, trajectories and records on the cases
of tests/prologue_cases.py (the control copy of phase 0 and the set-up of the gamma and theta waves).  Needs a GPU.

    ROVMPC_LIB=/path/to/librovmpc.so python tools/make_prologue_golden.py --commit <hash of the commit the library was built from>

Where a load is issued, and on which side of a barrier a value that does not depend on that barrier is computed, does not
enter any result's arithmetic, so a change to the prologue must leave every byte where it was: record the file from the
PARENT of such a change (the library ROVMPC_LIB names), never from the change itself."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rovmpc as rv  # noqa: E402
from plan_golden_cases import save_fixture  # noqa: E402
from prologue_cases import all_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="commit the library under ROVMPC_LIB was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rollout_prologue.npz"))
    args = ap.parse_args()
    import torch
    out = {"meta/parent_commit": np.array(args.commit), "meta/version": np.array(rv.load_library().rovmpc_version().decode()),
           "meta/gfx": np.array(torch.cuda.get_device_properties(0).gcnArchName)}
    for prefix, thunk in all_cases(rv):
        for part, a in thunk().items():
            out[f"{prefix}/{part}"] = np.asarray(a)
        print(prefix, flush=True)
    save_fixture(args.out, out)
    print(f"{args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes, library {os.environ.get('ROVMPC_LIB', rv.LIB_PATH)}")


if __name__ == "__main__":
    main()
