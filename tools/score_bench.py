#!/usr/bin/env python3
"""rovmpc.score_rows against the loop the library offered before it: one SymbolicRegressor per row (a library handle each),
rovmpc_replay per (row, recording), R^2 in NumPy.

R = 37 (all generation-1 rows of tests/golden/equations.json, theta and gamma fronts together -- a timing workload; the
fronts are scored separately in use), T = 2048 synthetic scaled rows N(0, 1) on a non-uniform time grid, B = 1 and 8,
RK4 and Euler.

1. Wall time of one sweep (all rows on all recordings, scores on the host), the new call and the loop alternating, --reps
   times each after a warm-up; the handles of the loop are built before the clock starts.  The two R^2 tables are compared.
2. Device time of score_rows_kernel and of the replay kernels from a separate `rocprofv3 --kernel-trace` run (--kernel-only).
3. The resource-usage remarks of score_rows_kernel (compiled here with hipcc, no GPU needed).

Usage: python tools/score_bench.py [--reps 3] [--no-profile] [--json profiles/score_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rovmpc  # noqa: E402

T = 2048
BS = (1, 8)
INTEGRATORS = ("rk4", "euler")
KERNELS = ("score_rows_kernel", "replay_increments_kernel", "replay_cumsum_kernel")


def rows():
    e = json.load(open(os.path.join(ROOT, "tests", "golden", "equations.json")))
    return [r["sympy_format"] for key in ("dtheta_dt", "dgamma_dt") for r in e[key]["rows"]]


def recordings(B, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, T, 18))
    time_ = np.cumsum(rng.uniform(0.005, 0.03, (B, T)), axis=1)
    truth = 0.3 + np.cumsum(0.01 * rng.standard_normal((B, T)), axis=1)
    return X, time_, truth


def r2_numpy(y, e):
    d, c = y - e, y - y.mean()
    return 1.0 - (d @ d) / (c @ c)


class Sweep:
    def __init__(self, B):
        self.B, self.texts = B, rows()
        self.X, self.time, self.truth = recordings(B)
        self.models = [rovmpc.SymbolicRegressor(t) for t in self.texts]
        for m in self.models:
            m._pair(m)                                                    # the handle of every row, before any clock

    def new(self, integrator):
        t0 = time.perf_counter()
        s = rovmpc.score_rows(self.texts, self.X, self.time, self.truth, integrator=integrator)
        return (time.perf_counter() - t0) * 1e3, s.r2

    def loop(self, integrator):
        code = rovmpc.RK4 if integrator == "rk4" else rovmpc.EULER
        t0 = time.perf_counter()
        r2 = np.empty((len(self.models), self.B))
        for r, m in enumerate(self.models):
            e = m._pair(m)
            for b in range(self.B):
                est, _ = e.replay(self.X[b], self.time[b], self.truth[b, 0], self.truth[b, 0], code)
                r2[r, b] = r2_numpy(self.truth[b], est)
        return (time.perf_counter() - t0) * 1e3, r2


def compare(reps):
    res = {}
    for B in BS:
        sw = Sweep(B)
        for integ in INTEGRATORS:
            tag = f"B{B}_{integ}"
            (_, a), (_, b) = sw.new(integ), sw.loop(integ)                # warm-up, and the tables to compare
            with np.errstate(all="ignore"):
                res[f"{tag}_max_r2_difference"] = float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
            wn, wl = [], []
            for _ in range(reps):                                         # alternating
                wn.append(sw.new(integ)[0]); wl.append(sw.loop(integ)[0])
            res[f"{tag}_score_rows_wall_ms"] = wn
            res[f"{tag}_replay_loop_wall_ms"] = wl
            res[f"{tag}_speedup_of_medians"] = float(np.median(wl) / np.median(wn))
    return res


def kernel_only():
    for B in BS:
        sw = Sweep(B)
        for integ in INTEGRATORS:
            sw.new(integ); sw.loop(integ)


def profile():
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="score_prof_")
    cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "score", "--", sys.executable, os.path.abspath(__file__), "--kernel-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv"}
    spans = []
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            k = next((k for k in KERNELS if k in row["Kernel_Name"]), None)
            if k:
                spans.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
    spans.sort()
    # the run's order: for B, for integrator: one score_rows launch, then R B replays of two launches each (T > 1)
    out, i, R = {}, 0, len(rows())
    for B in BS:
        for integ in INTEGRATORS:
            want = [KERNELS[0]] + [KERNELS[1], KERNELS[2]] * (R * B)
            part = spans[i:i + len(want)]
            i += len(want)
            if [p[2] for p in part] != want:
                return {"profile": f"unexpected kernel order at B={B} {integ}", "dispatches": len(spans)}
            tag = f"B{B}_{integ}"
            out[f"{tag}_score_rows_kernel_us"] = (part[0][1] - part[0][0]) / 1e3
            out[f"{tag}_replay_kernels_us"] = sum(b - a for a, b, _ in part[1:]) / 1e3
            out[f"{tag}_replay_launches"] = len(part) - 1
    shutil.rmtree(d, ignore_errors=True)
    return out


def resource_usage():
    pkg = os.path.dirname(os.path.dirname(rovmpc.LIB_PATH))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return {"resource_usage": "hipcc not found"}
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
           "-c", "-o", os.devnull, os.path.join(pkg, "csrc", "helpers_host.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|SGPRs Spill|VGPRs Spill): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = "score_rows_kernel" if "score_rows_kernel" in m.group(2) else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--resource-usage-only", action="store_true", help="no GPU needed; merged into an existing --json file")
    ap.add_argument("--no-resource-usage", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.kernel_only:
        kernel_only()
        return
    if a.resource_usage_only:
        out = json.load(open(a.json)) if a.json and os.path.exists(a.json) else {}
        out["resource_usage"] = resource_usage()
    else:
        out = {"R": len(rows()), "T": T, "B": list(BS), "tile": rovmpc._lib.SCORE_TILE}
        out.update(compare(a.reps))
        if not a.no_profile:
            out["kernels"] = profile()
        if not a.no_resource_usage:
            out["resource_usage"] = resource_usage()
    for k, v in out.items():
        print(f"{k:40s} : {v}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
