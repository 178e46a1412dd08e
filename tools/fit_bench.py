#!/usr/bin/env python3
"""The marker fit (rovmpc_fit_theta_gamma) at M = 16 markers, default configuration (L = 3 m, bracket (1e-6, 10), ENU).

Frames: P0 = 0, P1 = the vehicle of rovmpc.synthetic_problem moved by 0.2 m Gaussian, (theta, gamma) uniform in +-0.3 rad, the
markers from rovmpc_transform_catenary (frames whose cable is the chord are drawn again), with and without 1 mm Gaussian noise
on the interior markers; every fit starts from (0, 0).

1. Host-clock microseconds per call of the host entry (uploads, one launch, one synchronise, the copy back) for B = 1, 64 and
   4096 noisy frames, one prepared ctypes call each, and the mean trial steps and status counts of the noise-free and noisy
   sets (B = 4096).
2. Device time of fit_theta_gamma_kernel from a separate `rocprofv3 --kernel-trace --stats` run of this script
   (--kernel-only): 100 calls at each B in that order, averaged per B from the trace's dispatch rows in launch order.

Usage: python tools/fit_bench.py [--calls 300] [--no-profile] [--json OUT] [--stats-csv OUT]
"""
import argparse
import csv
import ctypes as C
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

M = 16
BS = (1, 64, 4096)
PROFILE_CALLS = 100


def frames(B, noise, seed=7):
    """(P0, P1, Y (B, M, 3), truth (B, 2)) of B frames whose cable is a catenary."""
    rng = np.random.default_rng(seed)
    e = rovmpc.default_engine()
    state, _ = rovmpc.synthetic_problem(1, 1)
    P1s, Ys, ts = [], [], []
    have = 0
    while have < B:
        n = B - have + 16
        P1 = state[3:6] + 0.2 * rng.standard_normal((n, 3))
        t = rng.uniform(-0.3, 0.3, (n, 2))
        out, npts, _ = e.transform_catenary(np.zeros((n, 3)), P1, t[:, 0], t[:, 1], e.cfg.L, M)
        ok = npts[:, 1] == M
        P1s.append(P1[ok]); Ys.append(out[3][ok]); ts.append(t[ok])
        have += int(ok.sum())
    P1, Y, t = (np.concatenate(x)[:B] for x in (P1s, Ys, ts))
    Y = Y.copy()
    if noise:
        Y[:, 1:-1] += noise * rng.standard_normal((B, M - 2, 3))
    return np.zeros((B, 3)), np.ascontiguousarray(P1), np.ascontiguousarray(Y), t


def call_of(e, P0, P1, Y):
    out = np.empty((len(Y), 6))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    args = (e._h, ptr(P0), ptr(P1), ptr(Y), len(Y), M, None, None, ptr(out))
    return (lambda: e.lib.rovmpc_fit_theta_gamma(*args)), out


def time_calls(calls):
    e = rovmpc.default_engine()
    res = {}
    for noise, tag in ((0.0, "noise_free"), (1e-3, "noisy")):
        P0, P1, Y, truth = frames(BS[-1], noise)
        fit = e.fit_theta_gamma(P0, P1, Y)
        conv = fit.status == rovmpc.FitStatus.CONVERGED
        res[f"{tag}_mean_trial_steps"] = float(fit.iters[conv].mean())
        res[f"{tag}_max_trial_steps"] = int(fit.iters.max())
        res[f"{tag}_status_counts"] = {s.name: int((fit.status == s).sum()) for s in rovmpc.FitStatus if (fit.status == s).any()}
        err = np.abs(np.stack([fit.theta, fit.gamma], axis=1) - truth)[conv]
        res[f"{tag}_max_angle_error_rad"] = float(err.max())
    for B in BS:
        fn, _ = call_of(e, P0[:B], P1[:B], Y[:B])
        for _ in range(20):
            assert fn() == 0
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        res[f"host_call_B{B}_us"] = (time.perf_counter() - t0) / calls * 1e6
    return res


def kernel_only():
    e = rovmpc.default_engine()
    P0, P1, Y, _ = frames(BS[-1], 1e-3)
    for B in BS:
        fn, _ = call_of(e, P0[:B], P1[:B], Y[:B])
        for _ in range(PROFILE_CALLS):
            assert fn() == 0


def profile(stats_csv):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="fit_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fit", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv"}
    rows = []
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            if "fit_theta_gamma_kernel" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort()
    out = {"fit_kernel_dispatches": len(rows)}
    if len(rows) == len(BS) * PROFILE_CALLS:
        for i, B in enumerate(BS):
            part = rows[i * PROFILE_CALLS:(i + 1) * PROFILE_CALLS]
            out[f"fit_kernel_B{B}_us"] = float(np.mean([(t1 - t0) / 1e3 for t0, t1 in part]))
    if stats_csv and stats:
        os.makedirs(os.path.dirname(os.path.abspath(stats_csv)), exist_ok=True)
        shutil.copyfile(stats[0], stats_csv)
    shutil.rmtree(d, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--stats-csv", default=None)
    a = ap.parse_args()
    if a.kernel_only:
        kernel_only()
        return
    out = {"M": M, "L": rovmpc.MPCConfig().L, "bracket": [rovmpc.MPCConfig().c_lo, rovmpc.MPCConfig().c_hi], "calls": a.calls}
    out.update(time_calls(a.calls))
    if not a.no_profile:
        out["kernels"] = profile(a.stats_csv)
    for k, v in out.items():
        print(f"{k:32s} : {v}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
