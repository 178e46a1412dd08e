#!/usr/bin/env python3
"""The cable-length calibration (rovmpc_calibrate_cable) at G = 1 and M = 16 markers: one cable, one recording, on an engine
with L = 3 m and the bracket (1e-6, 200) (a trial at which ANY frame leaves the bracket is a rejected step for the whole
group: with the default c_hi = 10 a long recording of these frames always holds one that is close to it).

Frames as in tests/calib_reference.recording: chord radius 0.8..1.8 m, z +-0.6 m, theta +-0.3, gamma +-0.4, the markers of a
2.7 m cable from rovmpc_cable_markers with 1 mm Gaussian noise, starts 0.1 rad off, L0 = 3 m, tolerances 1e-9.  Two
placements: markers by arc length fitted by arc length, and markers by the index rule fitted by the index rule.

1. Host-clock milliseconds per call of the host entry (uploads, the launch pairs in batches of 8 with a look at the done
   words in between, the copy back) and of the device entry (max_iter + 1 launch pairs enqueued, one synchronise) at 256,
   2048 and 16384 frames; the trial steps used; the same with free_length = 0 (the frames kernel then makes one model
   evaluation per trial instead of two).
2. Device time per launch of calib_frames_kernel and calib_reduce_kernel from separate `rocprofv3 --kernel-trace` runs of
   this script (--kernel-only --placement arc|index), averaged over the launches that did work (a launch of an ended group returns at once and is
   counted apart).
3. scipy.optimize.least_squares (method "trf", sparse Jacobian structure, NumPy forward model) on the 256-frame problem from the
   same start, host seconds, for comparison.

Usage: python tools/calib_bench.py [--calls 20] [--no-profile] [--no-scipy] [--json OUT]
"""
import argparse
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

M = 16
FS = (256, 2048, 16384)
L_TRUE, L0, TOL, NOISE = 2.7, 3.0, 1e-9, 1e-3


def recording(e, n, arc, seed=7):
    rng = np.random.default_rng(seed)
    rad, az = rng.uniform(0.8, 1.8, n), rng.uniform(0, 2 * np.pi, n)
    P1 = np.stack([rad * np.cos(az), rad * np.sin(az), rng.uniform(-0.6, 0.6, n)], axis=1)
    P0 = np.zeros((n, 3))
    th, ga = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.4, 0.4, n)
    Y = e.cable_markers(P0, P1, th, ga, L=np.full(n, L_TRUE), arc=arc, M=M)
    Y[:, 1:-1] += NOISE * rng.standard_normal((n, M - 2, 3))
    guess = np.stack([th, ga], axis=1) + 0.1 * rng.choice([-1.0, 1.0], (n, 2))
    return P0, P1, Y, guess


def engine():
    return rovmpc.Engine(rovmpc.MPCConfig(N=1, K=1, c_lo=1e-6, c_hi=200.0))


def time_calls(calls):
    e = engine()
    res = {}
    for tag, arc in (("arc", np.arange(M) / (M - 1.0)), ("index", None)):
        for n in FS:
            P0, P1, Y, guess = recording(e, n, arc)
            for free in (True, False):
                kw = dict(guess=guess, arc=arc, L0=L0 if free else L_TRUE, free_length=free, tol=TOL, tol_L=TOL)
                key = f"{tag}_F{n}" + ("" if free else "_fixedL")
                for device in (False, True):
                    og, _ = e.calibrate_cable(P0, P1, Y, [0, n], device=device, **kw)
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        e.calibrate_cable(P0, P1, Y, [0, n], device=device, **kw)
                    res[f"{key}_{'device' if device else 'host'}_call_ms"] = (time.perf_counter() - t0) / calls * 1e3
                res[f"{key}_trial_steps"] = int(og[0, 4])
                res[f"{key}_status"] = rovmpc.CalibStatus(int(og[0, 5])).name
                res[f"{key}_L"] = float(og[0, 0])
                res[f"{key}_sigma_L"] = float(og[0, 3])
    return res


def kernel_only(placement):
    e = engine()
    arc = np.arange(M) / (M - 1.0) if placement == "arc" else None
    for n in FS:
        P0, P1, Y, guess = recording(e, n, arc)
        for free in (True, False):
            for _ in range(5):
                e.calibrate_cable(P0, P1, Y, [0, n], guess=guess, arc=arc, L0=L0 if free else L_TRUE, free_length=free, tol=TOL, tol_L=TOL)


def profile(placement):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="calib_prof_")
    cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "calib", "--", sys.executable, os.path.abspath(__file__), "--kernel-only", "--placement", placement]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv"}
    rows = []
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            for k in ("calib_frames_kernel", "calib_reduce_kernel"):
                if k in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), k, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3,
                                 int(row.get("Grid_Size", row.get("Grid_Size_X", 0)) or 0)))
    rows.sort()
    out = {"dispatches": len(rows)}
    # the launches of one call: the frames kernel's grid tells the frame count; launches of an ended group are the short tail
    for n in FS:
        grid = (n + 3) // 4 * 256
        fr = [us for _, k, us, g in rows if k == "calib_frames_kernel" and g == grid]
        if not fr:
            continue
        live = [us for us in fr if us > 0.5 * np.median(sorted(fr)[-max(1, len(fr) // 4):])]
        out[f"frames_kernel_F{n}_us"] = float(np.mean(live))
        out[f"frames_kernel_F{n}_live_launches"] = len(live)
        out[f"frames_kernel_F{n}_ended_us"] = float(np.mean([us for us in fr if us not in live])) if len(live) < len(fr) else None
    red = [us for _, k, us, _ in rows if k == "calib_reduce_kernel"]
    out["reduce_kernel_all_us_min_median_max"] = [float(np.min(red)), float(np.median(red)), float(np.max(red))] if red else None
    # the reduce kernel follows its frames kernel: pair them up to get it per frame count
    prev = None
    per = {n: [] for n in FS}
    for _, k, us, g in rows:
        if k == "calib_frames_kernel":
            prev = g
        elif prev is not None:
            for n in FS:
                if prev == (n + 3) // 4 * 256:
                    per[n].append(us)
    for n in FS:
        if per[n]:
            top = sorted(per[n])[-max(1, len(per[n]) // 4):]
            out[f"reduce_kernel_F{n}_us"] = float(np.median(top))
    shutil.rmtree(d, ignore_errors=True)
    return out


def scipy_compare(n=256):
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import calib_reference as cf
    e = engine()
    arc = np.arange(M) / (M - 1.0)
    P0, P1, Y, guess = recording(e, n, arc)
    bracket = (e.cfg.c_lo, e.cfg.c_hi)

    def resid(x):
        X, _, _ = cf.model_vec(P1 - P0, x[1:n + 1], x[n + 1:], x[0], M, 1.0, bracket, arc)
        return (X - (Y - P0[:, None, :])).reshape(-1)

    S = lil_matrix((n * M * 3, 2 * n + 1), dtype=int)
    S[:, 0] = 1
    for f in range(n):
        S[f * M * 3:(f + 1) * M * 3, 1 + f] = 1
        S[f * M * 3:(f + 1) * M * 3, 1 + n + f] = 1
    x0 = np.concatenate([[L0], guess[:, 0], guess[:, 1]])
    t0 = time.perf_counter()
    r = least_squares(resid, x0, jac_sparsity=S, method="trf", xtol=1e-12, ftol=1e-15, gtol=1e-15)
    dt = time.perf_counter() - t0
    og, of = e.calibrate_cable(P0, P1, Y, [0, n], guess=guess, arc=arc, L0=L0, tol=TOL, tol_L=TOL)
    return {"scipy_F": n, "scipy_seconds": dt, "scipy_nfev": int(r.nfev), "scipy_L": float(r.x[0]), "scipy_minus_gpu_L": float(r.x[0] - og[0, 0]),
            "scipy_minus_gpu_max_angle": float(max(np.abs(r.x[1:n + 1] - of[:, 0]).max(), np.abs(r.x[n + 1:] - of[:, 1]).max()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--placement", choices=("arc", "index"), default="arc")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.kernel_only:
        kernel_only(a.placement)
        return
    out = {"M": M, "L_true": L_TRUE, "L0": L0, "noise_m": NOISE, "tol": TOL, "calls": a.calls}
    out.update(time_calls(a.calls))
    if not a.no_scipy:
        out.update(scipy_compare())
    if not a.no_profile:
        out["kernels"] = profile("arc")
        out["kernels_index"] = profile("index")
    for k, v in out.items():
        print(f"{k:40s} : {v}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
