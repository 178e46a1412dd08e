#!/usr/bin/env python3
"""MPPI against the shooting step at C2 (N = 20, K = 4096, fp64).

1. Host-clock microseconds per control step (one prepared ctypes call each, >= 500 steps after warm-up) of
   rovmpc_mppi_step with n_iter = 1, 2, 4 next to rovmpc_mpc_step_sampled, in one process.
2. The update kernel's device time from a separate `rocprofv3 --kernel-trace --stats` run of this script (--kernel-only),
   with its algorithmic bytes K (3N + 1) sizeof(T) and the GB/s they imply; the sampler's and the rollout's times too.
3. A 500-step host-fed loop over the measured rows of Rov_traj_gen case 12 (closed_loop_inputs): the shooting controller
   (MPC, device sampling) against MPPI, mean J* and sum |u_t - u_{t-1}|.  Reported, not asserted.

Usage: python tools/mppi_bench.py [--steps 2000] [--no-profile] [--json OUT]
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
from rovmpc.closed_loop import closed_loop_inputs  # noqa: E402

N, K = 20, 4096


def pick_lambda(state, std):
    """A temperature on the scale of the spread of the costs of one draw around the default nominal."""
    m = rovmpc.MPPI(N=N, K=K, lam=1.0, std=std, n_iter=1)
    m.step(state)
    _, J = m.engine.mppi_last()
    m.close()
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


def time_steps(steps, lam, std, state):
    out = {}
    # the shooting step, fused sampling (one library call)
    mpc = rovmpc.MPC(N=N, K=K, device_sampling=True)
    eng = mpc.engine
    m = rovmpc.default_model()
    for i in range(50):
        eng.mpc_step_sampled(state, 1, i, m.mean[3:6], m.scale[3:6], True)
    sp = eng._samp
    fn = eng.lib.rovmpc_mpc_step_sampled
    t0 = time.perf_counter()
    for i in range(steps):
        fn(eng._h, sp["pstate"], 1, i, sp["pm"], sp["ps"], 1, sp["prec"])
    out["mpc_step_sampled_us"] = (time.perf_counter() - t0) / steps * 1e6
    mpc.close()
    for I in (1, 2, 4):
        ctl = rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=I)
        e = ctl.engine
        st = State()
        C.memmove(C.byref(st), np.ascontiguousarray(state, np.float64).ctypes.data, 128)
        rec, nu, stats = np.empty(e.result_len), np.empty((N, 3)), np.empty(4)
        args = (C.byref(st), C.byref(ctl.params), rec.ctypes.data_as(C.c_void_p), nu.ctypes.data_as(C.c_void_p),
                stats.ctypes.data_as(C.c_void_p))
        fn = e.lib.rovmpc_mppi_step
        for i in range(50):
            assert fn(e._h, args[0], 7, i, args[1], args[2], args[3], args[4]) == 0
        t0 = time.perf_counter()
        for i in range(steps):
            fn(e._h, args[0], 7, 50 + i, args[1], args[2], args[3], args[4])
        out[f"mppi_I{I}_us"] = (time.perf_counter() - t0) / steps * 1e6
        ctl.close()
    return out


def kernel_only(lam, std, state, steps=300):
    ctl = rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=1)
    for _ in range(steps):
        ctl.step(state)
    ctl.close()


def profile(lam, std):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="mppi_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mppi", "--", sys.executable, os.path.abspath(__file__),
           "--kernel-only", "--lam", repr(lam), "--std", *[repr(float(v)) for v in std]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"profile": "no kernel_stats.csv among " + " ".join(os.path.relpath(f, d) for f in glob.glob(os.path.join(d, "**"), recursive=True))[:400]}
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            avg = float(row.get("AverageNs", row.get("AverageNS", "nan")))
            calls = int(row.get("Calls", 0))
            for key, pat in (("update", "mppi_update_kernel"), ("sample", "mppi_sample_kernel"), ("rollout", "rollout_kernel")):
                if pat in name and f"{key}_us" not in out:
                    out[f"{key}_us"] = avg / 1e3
                    out[f"{key}_calls"] = calls
    shutil.rmtree(d, ignore_errors=True)
    if "update_us" in out:
        out["update_bytes"] = K * (3 * N + 1) * 8
        out["update_GBps"] = out["update_bytes"] / (out["update_us"] * 1e-6) / 1e9
    return out


def loop(lam, std, n_steps=500):
    mpc = rovmpc.MPC(N=N, K=K, device_sampling=True)
    rows, _ = closed_loop_inputs(mpc.engine, 12, n_steps)
    ctl = rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=1)
    res = {}
    for name, c in (("shooting", mpc), ("mppi", ctl)):
        us, Js = [], []
        for r in rows:
            us.append(c.step(r).copy())
            Js.append(c.last.cost)
        us = np.array(us)
        Js = np.array(Js)
        fin = np.isfinite(Js)
        res[name] = {"mean_J_star": float(Js[fin].mean()) if fin.any() else float("nan"), "finite_steps": int(fin.sum()),
                     "sum_du": float(np.linalg.norm(np.diff(us, axis=0), axis=1).sum())}
    if ctl.last_stats:
        res["mppi"]["last_ess"] = ctl.last_stats["ess"]
    mpc.close(); ctl.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--lam", type=float, default=None)
    ap.add_argument("--std", type=float, nargs=3, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    model = rovmpc.default_model()
    std = np.asarray(a.std if a.std else model.scale[3:6], dtype=np.float64)
    state, _ = rovmpc.synthetic_problem(1, N)
    lam = a.lam if a.lam is not None else pick_lambda(state, std)
    if a.kernel_only:
        kernel_only(lam, std, state)
        return
    out = {"N": N, "K": K, "dtype": "f64", "lambda": lam, "steps": a.steps}
    out.update(time_steps(max(a.steps, 500), lam, std, state))
    out["mppi_I1_over_sampled"] = out["mppi_I1_us"] / out["mpc_step_sampled_us"]
    print(f"rovmpc_mpc_step_sampled          : {out['mpc_step_sampled_us']:8.2f} us/step")
    for I in (1, 2, 4):
        print(f"rovmpc_mppi_step, n_iter = {I}     : {out[f'mppi_I{I}_us']:8.2f} us/step")
    print(f"MPPI (I = 1) / sampled step      : {out['mppi_I1_over_sampled']:8.2f}x")
    if not a.no_profile:
        p = profile(lam, std)
        out["kernels"] = p
        if "update_us" in p:
            print(f"mppi_update_kernel               : {p['update_us']:8.2f} us  ({p['update_bytes'] / 1e6:.2f} MB, "
                  f"{p['update_GBps']:.0f} GB/s)")
            print(f"mppi_sample_kernel               : {p.get('sample_us', float('nan')):8.2f} us")
            print(f"rollout kernel                   : {p.get('rollout_us', float('nan')):8.2f} us")
        else:
            print("profile:", p)
    out["loop_case12"] = loop(lam, std)
    for name, r in out["loop_case12"].items():
        print(f"case 12, 500 steps, {name:9s}: mean J* {r['mean_J_star']:.6g}, sum |du| {r['sum_du']:.6g}, "
              f"finite steps {r['finite_steps']}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
