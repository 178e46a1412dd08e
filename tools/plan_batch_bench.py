#!/usr/bin/env python3
"""Batched MPPI and CEM at C2 (N = 20, K = 4096, fp64): one library call advances B plans.

1. Host-clock microseconds per control step (one prepared ctypes call each, >= 300 steps after warm-up) of
   rovmpc_mppi_step_batch and rovmpc_cem_step_batch for B in {1, 2, 8, 32, 64} and n_iter in {1, 2}, per call and per problem,
   next to the single-problem rovmpc_mppi_step / rovmpc_cem_step of the same process (--single-repeats runs of each, so the
   spread of that number is on the page).
2. Kernel times of the batched samplers, rollouts and updates from a separate `rocprofv3 --kernel-trace --stats` run of this
   script (--kernel-only B), per launch and per problem.

3. --single-only: the single-problem steps alone, which an older build of the library has too -- the A/B of a commit against
   its parent: ROVMPC_LIB=<pkg>/lib/librovmpc_<name>.so ROVMPC_LIB_OLD_ABI=1 python tools/plan_batch_bench.py --single-only,
   once per library and turn, interleaved (the way tools/ab_libs.sh does it for the rollout).

Usage: python tools/plan_batch_bench.py [--steps 1000] [--no-profile] [--profile-B 1 64] [--stats-out DIR] [--json OUT]
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
BATCHES = (1, 2, 8, 32, 64)
ITERS = (1, 2)
P = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(P)


def states_of(B):
    state, _ = rovmpc.synthetic_problem(1, N)
    st = np.tile(state, (B, 1))
    st[:, 12] += 1e-3 * np.arange(B)
    return np.ascontiguousarray(st)


def pick_lambda(std):
    m = rovmpc.MPPI(N=N, K=K, lam=1.0, std=std, n_iter=1)
    m.step(states_of(1)[0])
    _, J = m.engine.mppi_last()
    m.close()
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


def controller(kind, B, I, lam, std):
    if kind == "mppi":
        return rovmpc.BatchedMPPI(N=N, K=K, B=B, lam=lam, std=std, n_iter=I)
    return rovmpc.BatchedCEM(N=N, K=K, B=B, n_elite=64, n_iter=I, std=std)


def time_batched(kind, B, I, lam, std, steps):
    ctl = controller(kind, B, I, lam, std)
    e = ctl.engine
    st, seeds = states_of(B), ctl.seeds
    rec = np.empty((B, e.result_len))
    if kind == "mppi":
        fn = e.lib.rovmpc_mppi_step_batch
        call = lambda s: fn(e._h, B, ptr(st), ptr(seeds), s, C.byref(ctl.params), ptr(rec), None, None)          # noqa: E731
    else:
        fn = e.lib.rovmpc_cem_step_batch
        call = lambda s: fn(e._h, B, ptr(st), ptr(seeds), s, C.byref(ctl.params), ptr(rec), None, None, None, None)   # noqa: E731
    for s in range(30):
        assert call(s) == 0
    t0 = time.perf_counter()
    for s in range(steps):
        call(30 + s)
    us = (time.perf_counter() - t0) / steps * 1e6
    ctl.close()
    return us


def time_single(kind, I, lam, std, steps):
    ctl = rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=I) if kind == "mppi" else rovmpc.CEM(N=N, K=K, n_elite=64, n_iter=I, std=std)
    e = ctl.engine
    s0 = State()
    C.memmove(C.byref(s0), states_of(1).ctypes.data, 128)
    rec = np.empty(e.result_len)
    if kind == "mppi":
        fn = e.lib.rovmpc_mppi_step
        call = lambda s: fn(e._h, C.byref(s0), 7, s, C.byref(ctl.params), ptr(rec), None, None)                  # noqa: E731
    else:
        fn = e.lib.rovmpc_cem_step
        call = lambda s: fn(e._h, C.byref(s0), 7, s, C.byref(ctl.params), ptr(rec), None, None, None, None)     # noqa: E731
    for s in range(50):
        assert call(s) == 0
    t0 = time.perf_counter()
    for s in range(steps):
        call(50 + s)
    us = (time.perf_counter() - t0) / steps * 1e6
    ctl.close()
    return us


def kernel_only(B, lam, std, steps=100):
    for kind in ("mppi", "cem"):
        ctl = controller(kind, B, 1, lam, std)
        st = states_of(B)
        for _ in range(steps):
            ctl.step(st)
        ctl.close()


KERNELS = (("mppi_sample", "mppi_sample_batch_kernel"), ("mppi_update", "mppi_update_batch_kernel"),
           ("cem_sample", "cem_sample_batch_kernel"), ("cem_update", "cem_update_batch_kernel"), ("rollout", "rollout_kernel"))


def profile(B, lam, std, stats_out=None):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="plan_batch_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "plan_batch", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-only", str(B), "--lam", repr(lam), "--std", *[repr(float(v)) for v in std]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"profile": "no kernel_stats.csv"}
    out = {"B": B}
    if stats_out:
        os.makedirs(stats_out, exist_ok=True)
        shutil.copy(files[0], os.path.join(stats_out, f"plan_batch_kernel_stats_B{B}.csv"))
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            avg = float(row.get("AverageNs", row.get("AverageNS", "nan")))
            for key, pat in KERNELS:
                if pat in name and f"{key}_us" not in out:
                    out[f"{key}_us"] = avg / 1e3
                    out[f"{key}_calls"] = int(row.get("Calls", 0))
    shutil.rmtree(d, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--single-repeats", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-B", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--stats-out", default=None, metavar="DIR", help="keep rocprofv3's kernel_stats.csv of each profiled B here")
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--kernel-only", type=int, default=0, metavar="B")
    ap.add_argument("--lam", type=float, default=None)
    ap.add_argument("--std", type=float, nargs=3, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    std = np.asarray(a.std if a.std else rovmpc.default_model().scale[3:6], dtype=np.float64)
    lam = a.lam if a.lam is not None else pick_lambda(std)
    if a.kernel_only:
        kernel_only(a.kernel_only, lam, std)
        return
    out = {"N": N, "K": K, "dtype": "f64", "lambda": lam, "steps": a.steps, "single": {}, "batched": {}}
    for kind in ("mppi", "cem"):
        for I in ITERS:
            runs = [time_single(kind, I, lam, std, max(a.steps, 300)) for _ in range(a.single_repeats)]
            out["single"][f"{kind}_I{I}_us"] = runs
            print(f"rovmpc_{kind}_step, n_iter = {I}: " + ", ".join(f"{v:7.2f}" for v in runs) + " us/step")
    if a.single_only:
        out["lib"] = os.environ.get("ROVMPC_LIB", "in-tree")
        print(json.dumps(out))
        return
    print(f"{'':22s}{'B':>4s} {'us/call':>10s} {'us/problem':>11s}  single/per-problem")
    for kind in ("mppi", "cem"):
        for I in ITERS:
            single = min(out["single"][f"{kind}_I{I}_us"])
            for B in BATCHES:
                us = time_batched(kind, B, I, lam, std, max(a.steps // max(B // 8, 1), 300))
                out["batched"][f"{kind}_I{I}_B{B}_us"] = us
                print(f"{kind}_step_batch, I = {I}   {B:4d} {us:10.2f} {us / B:11.2f}  {single / (us / B):6.2f}x")
    if not a.no_profile:
        out["kernels"] = []
        for pB in a.profile_B:
            p = profile(pB, lam, std, a.stats_out)
            out["kernels"].append(p)
            if "rollout_us" in p:
                for key, _ in KERNELS:
                    if f"{key}_us" in p:
                        print(f"{key:12s} B = {p['B']:3d}: {p[f'{key}_us']:9.2f} us/launch {p[f'{key}_us'] / p['B']:8.2f} us/problem "
                              f"({p[f'{key}_calls']} launches)")
            else:
                print("profile:", p)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
