#!/usr/bin/env python3
"""Record tests/golden/helper_entries.npz: the bits of the host-pointer helper entries (rovmpc_predict ...
rovmpc_kabsch_velocity_transform, rovmpc_math_probe) on the cases of tests/helper_golden_cases.py.  Needs a GPU.

    ROVMPC_LIB=/path/to/librovmpc.so python tools/make_helper_golden.py --commit <hash of the commit the library was built from>

The library is the one ROVMPC_LIB names (rovmpc/_lib.py), so the fixture can be taken from the parent of a change to the host
code that must not move a bit.  The file also holds the commit, rovmpc_version() and the gfx target."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rovmpc as rv  # noqa: E402
from helper_golden_cases import OK, call, cases, handle, last_error, save_fixture  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="commit the library under ROVMPC_LIB was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "helper_entries.npz"))
    args = ap.parse_args()
    import torch
    out = {"meta/parent_commit": np.array(args.commit), "meta/version": np.array(rv.load_library().rovmpc_version().decode()),
           "meta/gfx": np.array(torch.cuda.get_device_properties(0).gcnArchName)}
    with handle(rv) as eng:
        for c in cases(rv):
            rc, outs = call(eng, c)
            if rc != OK:
                raise SystemExit(f"{c.name}: status {rc}: {last_error(eng)}")
            for name, a in outs.items():
                out[f"{c.name}/{name}"] = a
            print(c.name, flush=True)
    save_fixture(args.out, out)
    print(f"{args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes, library {os.environ.get('ROVMPC_LIB', rv.LIB_PATH)}")


if __name__ == "__main__":
    main()
