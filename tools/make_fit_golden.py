#!/usr/bin/env python3
"""Record tests/golden/fit_entries.npz: the bits of rovmpc_fit_theta_gamma on tests/fit_reference.scenes(), each from its
own start and from every start of the tracker's default list.  Needs a GPU.

    ROVMPC_LIB=/path/to/librovmpc.so python tools/make_fit_golden.py --commit <hash of the commit the library was built from>

The library is the one ROVMPC_LIB names (rovmpc/_lib.py), so the fixture is taken from the parent of a change to the fit's
device code that must not move a bit (tests/test_fit_golden_gpu.py).  The file also holds the commit, rovmpc_version() and
the gfx target."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rovmpc as rv  # noqa: E402
import fit_golden_cases as fg  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="commit the library under ROVMPC_LIB was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fit_entries.npz"))
    args = ap.parse_args()
    import torch
    out = {"meta_parent_commit": np.array(args.commit), "meta_version": np.array(rv.load_library().rovmpc_version().decode()),
           "meta_gfx": np.array(torch.cuda.get_device_properties(0).gcnArchName)}
    out.update(fg.run(rv))
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes, library {os.environ.get('ROVMPC_LIB', rv.LIB_PATH)}")


if __name__ == "__main__":
    main()
