#!/usr/bin/env python3
"""Record tests/golden/plan_controllers.npz: the bits of the MPPI / CEM controller entry points (single, batched, device
loops, *_update_device) on the cases of tests/plan_golden_cases.py.  Needs a GPU.

    ROVMPC_LIB=/path/to/librovmpc.so python tools/make_plan_golden.py --commit <hash of the commit the library was built from>

The library is the one ROVMPC_LIB names (rovmpc/_lib.py), so the fixture can be taken from the parent of a change that must
not move a bit; a change to the kernels that legitimately moves bits records it again from its own build.  The file also
holds the commit, rovmpc_version(), the gfx target and the MPPI temperatures measured for the cases."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rovmpc as rv  # noqa: E402
from plan_golden_cases import CASES, lam_key, measure_lam, run_case, save_fixture  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="commit the library under ROVMPC_LIB was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plan_controllers.npz"))
    args = ap.parse_args()
    import torch
    out = {"meta/parent_commit": np.array(args.commit), "meta/version": np.array(rv.load_library().rovmpc_version().decode()),
           "meta/gfx": np.array(torch.cuda.get_device_properties(0).gcnArchName)}
    for c in CASES:
        if lam_key(c) not in out:
            out[lam_key(c)] = np.array(measure_lam(rv, c))
        for part, a in run_case(rv, c, float(out[lam_key(c)])).items():
            out[f"{c.name}/{part}"] = np.asarray(a)
        print(c.name, flush=True)
    save_fixture(args.out, out)
    print(f"{args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes, library {os.environ.get('ROVMPC_LIB', rv.LIB_PATH)}")


if __name__ == "__main__":
    main()
