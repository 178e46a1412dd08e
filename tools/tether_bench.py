#!/usr/bin/env python3
"""The tether keep-out cost of MPPI and CEM (rovmpc_set_tether_cost) at C2 (N = 20, K = 4096, fp64, the default
n_shape_pts, n_iter = 1, 2 spheres beside the initial cable).

1. Host-clock microseconds per control step (one prepared ctypes call each, >= 500 steps after warm-up) of rovmpc_mppi_step
   and rovmpc_cem_step without and with a tether cost, in one process: the step's total price, the rollout's slow tail
   (it stores all K trajectories) and the extra launch together.
2. Device times from a separate `rocprofv3 --kernel-trace --stats` run of this script (--kernel-only): 300 MPPI steps
   without the cost, then 300 with it.  The rollout kernel has one name in both halves, so its two averages (without and
   with the trajectory buffer) are taken from the trace's dispatch rows in launch order; tether_cost_kernel's average stands
   beside them.  --stats-csv keeps the trace's kernel_stats.csv.

Usage: python tools/tether_bench.py [--steps 2000] [--no-profile] [--json OUT] [--stats-csv OUT]
"""
import argparse
import ctypes as C
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rovmpc  # noqa: E402
from rovmpc._lib import State  # noqa: E402

N, K = 20, 4096
PROFILE_STEPS = 300


def bench_tether():
    """Two spheres of 0.1 m for the state of rovmpc.synthetic_problem, which this tool runs: beside its cable's mid-span (the
    steering test's sphere) and a quarter of the way down it."""
    return rovmpc.TetherCost([[0.0404, -0.4838, -1.1986, 0.10], [0.12, -0.25, -0.95, 0.10]], 1e4, margin=0.01)


def controller(kind, tether, std):
    if kind == "mppi":
        return rovmpc.MPPI(N=N, K=K, lam=1.0, std=std, n_iter=1, tether=tether)
    return rovmpc.CEM(N=N, K=K, std=std, n_iter=1, tether=tether)


def time_steps(steps, std, state):
    out = {}
    st = State()
    C.memmove(C.byref(st), np.ascontiguousarray(state, np.float64).ctypes.data, 128)
    for kind in ("mppi", "cem"):
        for setting, tether in (("plain", None), ("tether", bench_tether())):
            ctl = controller(kind, tether, std)
            e = ctl.engine
            bufs = [np.empty(e.result_len), np.empty((N, 3))]
            if kind == "cem":
                bufs += [np.empty((N, 3)), np.empty(ctl.n_elite, dtype=np.int64)]
            bufs.append(np.empty(4))
            ptrs = [b.ctypes.data_as(C.c_void_p) for b in bufs]
            fn = getattr(e.lib, f"rovmpc_{kind}_step")
            for i in range(50):
                assert fn(e._h, C.byref(st), 7, i, C.byref(ctl.params), *ptrs) == 0
            t0 = time.perf_counter()
            for i in range(steps):
                fn(e._h, C.byref(st), 7, 50 + i, C.byref(ctl.params), *ptrs)
            out[f"{kind}_{setting}_us"] = (time.perf_counter() - t0) / steps * 1e6
            ctl.close()
        out[f"{kind}_extra_us"] = out[f"{kind}_tether_us"] - out[f"{kind}_plain_us"]
    return out


def kernel_only(std, state):
    ctl = controller("mppi", None, std)
    for _ in range(PROFILE_STEPS):
        ctl.step(state)
    ctl.set_tether(bench_tether())
    for _ in range(PROFILE_STEPS):
        ctl.step(state)
    ctl.close()


def profile(std, stats_csv):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="tether_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tether", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-only", "--std", *[repr(float(v)) for v in std]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv among " + " ".join(os.path.relpath(f, d) for f in glob.glob(os.path.join(d, "**"), recursive=True))[:400]}
    rows = []
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    groups = {"rollout": [], "tether_cost": [], "mppi_sample": [], "mppi_update": []}
    for t0, t1, name in rows:
        for key in groups:
            if f"{key}_kernel" in name:
                groups[key].append((t1 - t0) / 1e3)
    out = {}
    ro = groups["rollout"]
    if len(ro) == 2 * PROFILE_STEPS:
        out["rollout_plain_us"] = float(np.mean(ro[:PROFILE_STEPS]))
        out["rollout_traj_buffer_us"] = float(np.mean(ro[PROFILE_STEPS:]))
        out["slow_tail_us"] = out["rollout_traj_buffer_us"] - out["rollout_plain_us"]
    else:
        out["rollout_dispatches"] = len(ro)
    for key in ("tether_cost", "mppi_sample", "mppi_update"):
        if groups[key]:
            out[f"{key}_us"] = float(np.mean(groups[key]))
            out[f"{key}_calls"] = len(groups[key])
    if "tether_cost_us" in out and "rollout_plain_us" in out:
        out["tether_over_rollout"] = out["tether_cost_us"] / out["rollout_plain_us"]
    if stats_csv and stats:
        os.makedirs(os.path.dirname(os.path.abspath(stats_csv)), exist_ok=True)
        shutil.copyfile(stats[0], stats_csv)
    shutil.rmtree(d, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--std", type=float, nargs=3, default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--stats-csv", default=None)
    a = ap.parse_args()
    model = rovmpc.default_model()
    std = np.asarray(a.std if a.std else model.scale[3:6], dtype=np.float64)
    state, _ = rovmpc.synthetic_problem(1, N)
    if a.kernel_only:
        kernel_only(std, state)
        return
    out = {"N": N, "K": K, "dtype": "f64", "n_shape_pts": rovmpc.MPCConfig().n_shape_pts, "spheres": 2, "steps": a.steps}
    out.update(time_steps(max(a.steps, 500), std, state))
    for kind in ("mppi", "cem"):
        for setting in ("plain", "tether"):
            print(f"rovmpc_{kind}_step, {setting:6s}         : {out[f'{kind}_{setting}_us']:8.2f} us/step")
        print(f"rovmpc_{kind}_step, extra          : {out[f'{kind}_extra_us']:8.2f} us/step")
    if not a.no_profile:
        p = profile(std, a.stats_csv)
        out["kernels"] = p
        for k, v in p.items():
            print(f"{k:32s} : {v if isinstance(v, (int, str)) else round(v, 3)}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
