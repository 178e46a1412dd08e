#!/usr/bin/env python3
"""rovmpc.score_pairs on the generation-1 fronts: all 23 x 14 = 322 pairs, H = 20, stride 1, T = 2048 synthetic scaled rows
N(0, 1) on a non-uniform time grid, B = 1 and 8, RK4 and Euler.

1. Wall time of one sweep through the host entry (uploads, one launch, the skill table on the host) and through the device
   entry (recordings already on the device; the call, the launch and the copy of the table back), --reps times each after a
   warm-up, alternating.  The library had no closed-loop scoring before, so the comparison is the NumPy restatement of the law
   (tests/horizon_reference.py, vectorised over the windows): timed on --np-pairs pairs of one recording and scaled to the
   sweep, which is stated in the result.  The two skill tables are compared on those pairs.
2. Device time of score_pairs_kernel from a separate `rocprofv3 --kernel-trace` run (--kernel-only).
3. The resource-usage remarks of score_pairs_kernel (compiled here with hipcc, no GPU needed).

Usage: python tools/horizon_bench.py [--reps 3] [--np-pairs 8] [--no-profile] [--json profiles/horizon_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import rovmpc  # noqa: E402

T, H, STRIDE = 2048, 20, 1
BS = (1, 8)
INTEGRATORS = ("rk4", "euler")
KERNEL = "score_pairs_kernel"


def fronts():
    e = json.load(open(os.path.join(ROOT, "tests", "golden", "equations.json")))
    return [[r["sympy_format"] for r in e[key]["rows"]] for key in ("dtheta_dt", "dgamma_dt")]


def scaler():
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "scaler.json")))
    return np.array(s["mean"], dtype=np.float64), np.array(s["scale"], dtype=np.float64)


def recordings(B, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, T, 18))
    time_ = np.cumsum(rng.uniform(0.005, 0.03, (B, T)), axis=1)
    theta = 0.3 + np.cumsum(0.01 * rng.standard_normal((B, T)), axis=1)
    gamma = -0.2 + np.cumsum(0.01 * rng.standard_normal((B, T)), axis=1)
    return X, time_, theta, gamma


class Sweep:
    def __init__(self, B):
        self.B = B
        self.theta_rows, self.gamma_rows = fronts()
        self.mean, self.scale = scaler()
        self.X, self.time, self.theta, self.gamma = recordings(B)

    def call(self, integrator, device, **kw):
        t0 = time.perf_counter()
        s = rovmpc.score_pairs(self.theta_rows, self.gamma_rows, self.X, self.time, self.theta, self.gamma, self.mean, self.scale, H,
                               stride=STRIDE, integrator=integrator, device=device, **kw)
        return (time.perf_counter() - t0) * 1e3, s

    def numpy(self, integrator, n_pairs):
        """(ms for n_pairs pairs on recording 0, their skill tables)."""
        import horizon_reference as hr
        integ = hr.RK4 if integrator == "rk4" else hr.EULER
        pairs = [(q % len(self.theta_rows), q % len(self.gamma_rows)) for q in range(n_pairs)]
        t0 = time.perf_counter()
        out = [hr.horizon_np(self.theta_rows[it], self.gamma_rows[ig], self.X[0], self.time[0], self.theta[0], self.gamma[0], self.mean, self.scale,
                             H, STRIDE, integ)[0] for it, ig in pairs]
        return (time.perf_counter() - t0) * 1e3, pairs, np.array(out)


def compare(reps, n_pairs):
    res = {}
    for B in BS:
        sw = Sweep(B)
        Q = len(sw.theta_rows) * len(sw.gamma_rows)
        for integ in INTEGRATORS:
            tag = f"B{B}_{integ}"
            (_, a), (_, b) = sw.call(integ, False), sw.call(integ, True)      # warm-up, and the tables to compare
            res[f"{tag}_device_entry_equals_host_entry"] = bool(np.array_equal(a.table(), b.table(), equal_nan=True))
            res[f"{tag}_pairs_counted_in_every_window_at_H"] = int((a.n_ok[:, :, -1] == a.windows[None, :]).all(axis=1).sum())
            wh, wd = [], []
            for _ in range(reps):                                             # alternating
                wh.append(sw.call(integ, False)[0]); wd.append(sw.call(integ, True)[0])
            res[f"{tag}_host_entry_wall_ms"] = wh
            res[f"{tag}_device_entry_wall_ms"] = wd
            if n_pairs:
                ms, pairs, ref = sw.numpy(integ, n_pairs)
                got = sw.call(integ, False, pairs=pairs)[1].table()[:, 0]
                with np.errstate(all="ignore"):
                    d = np.abs(got - ref) / np.maximum(1e-300, np.abs(ref))
                res[f"{tag}_numpy_ms_per_pair_recording"] = ms / n_pairs
                res[f"{tag}_numpy_sweep_ms_scaled_from_{n_pairs}_pairs"] = ms / n_pairs * Q * B
                res[f"{tag}_speedup_of_host_entry_over_numpy"] = float(ms / n_pairs * Q * B / np.median(wh))
                res[f"{tag}_max_relative_difference_to_numpy_where_small"] = float(np.nanmax(np.where(np.abs(ref) < 1e6, d, 0.0)))
    return res


def kernel_only():
    for B in BS:
        sw = Sweep(B)
        for integ in INTEGRATORS:
            sw.call(integ, False)


def profile():
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="horizon_prof_")
    cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "horizon", "--", sys.executable, os.path.abspath(__file__), "--kernel-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv"}
    spans = []
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            if KERNEL in row["Kernel_Name"]:
                spans.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    spans.sort()
    tags = [f"B{B}_{integ}" for B in BS for integ in INTEGRATORS]             # the run's order: one launch each
    if len(spans) != len(tags):
        return {"profile": f"expected {len(tags)} launches of {KERNEL}, saw {len(spans)}"}
    shutil.rmtree(d, ignore_errors=True)
    return {f"{tag}_{KERNEL}_us": (b - a) / 1e3 for tag, (a, b) in zip(tags, spans)}


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
            name = KERNEL if KERNEL in m.group(2) else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np-pairs", type=int, default=8, help="pairs the NumPy restatement is timed on (0: not at all)")
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
        out = {"pairs": 322, "T": T, "H": H, "stride": STRIDE, "B": list(BS), "tile": rovmpc._lib.HORIZON_TILE,
               "windows_per_recording": (T - 1 - H) // STRIDE + 1}
        out.update(compare(a.reps, a.np_pairs))
        if not a.no_profile:
            out["kernels"] = profile()
        if not a.no_resource_usage:
            out["resource_usage"] = resource_usage()
    for k, v in out.items():
        print(f"{k:56s} : {v}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
