#!/usr/bin/env python3
"""CEM against MPPI and the shooting step at C2 (N = 20, K = 4096, fp64, n_elite = 64).

1. Host-clock microseconds per control step (one prepared ctypes call each, >= 500 steps after warm-up) of
   rovmpc_cem_step with n_iter = 1, 2, 4 next to rovmpc_mppi_step (n_iter = 1) and rovmpc_mpc_step_sampled, in one process.
2. The device time of cem_update_kernel and cem_sample_kernel (and the rollout's) from a separate
   `rocprofv3 --kernel-trace --stats` run of this script (--kernel-only).
3. The 500-step host-fed loop of tools/mppi_bench.py over the measured rows of Rov_traj_gen case 12: shooting, MPPI and
   CEM, mean J* and sum |u_t - u_{t-1}|.  Reported, not asserted.

Usage: python tools/cem_bench.py [--steps 2000] [--no-profile] [--json OUT]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import rovmpc  # noqa: E402
from rovmpc._lib import State  # noqa: E402
from rovmpc.closed_loop import closed_loop_inputs  # noqa: E402
from mppi_bench import pick_lambda  # noqa: E402

N, K, E = 20, 4096, 64


def _timed(fn, steps, warm=50):
    for i in range(warm):
        assert fn(i) == 0
    t0 = time.perf_counter()
    for i in range(steps):
        fn(warm + i)
    return (time.perf_counter() - t0) / steps * 1e6


def time_steps(steps, lam, std, state):
    out = {}
    st = State()
    C.memmove(C.byref(st), np.ascontiguousarray(state, np.float64).ctypes.data, 128)
    m = rovmpc.default_model()
    # the shooting step, fused sampling (one library call)
    mpc = rovmpc.MPC(N=N, K=K, device_sampling=True)
    eng = mpc.engine
    eng.mpc_step_sampled(state, 1, 0, m.mean[3:6], m.scale[3:6], True)
    sp, fn = eng._samp, eng.lib.rovmpc_mpc_step_sampled
    out["mpc_step_sampled_us"] = _timed(lambda i: fn(eng._h, sp["pstate"], 1, i, sp["pm"], sp["ps"], 1, sp["prec"]), steps)
    mpc.close()
    ctl = rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=1)
    e = ctl.engine
    rec, nu, stats = np.empty(e.result_len), np.empty((N, 3)), np.empty(4)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fn = e.lib.rovmpc_mppi_step
    out["mppi_I1_us"] = _timed(lambda i: fn(e._h, C.byref(st), 7, i, C.byref(ctl.params), ptr(rec), ptr(nu), ptr(stats)), steps)
    ctl.close()
    for I in (1, 2, 4):
        ctl = rovmpc.CEM(N=N, K=K, n_elite=E, std=std, n_iter=I)
        e = ctl.engine
        rec, mu, sg, el, stats = np.empty(e.result_len), np.empty((N, 3)), np.empty((N, 3)), np.empty(E, np.int64), np.empty(4)
        fn = e.lib.rovmpc_cem_step
        out[f"cem_I{I}_us"] = _timed(lambda i: fn(e._h, C.byref(st), 7, i, C.byref(ctl.params), ptr(rec), ptr(mu), ptr(sg),
                                                  ptr(el), ptr(stats)), steps)
        ctl.close()
    return out


def kernel_only(std, state, steps=300):
    ctl = rovmpc.CEM(N=N, K=K, n_elite=E, std=std, n_iter=1)
    for _ in range(steps):
        ctl.step(state)
    ctl.close()


def profile(std):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="cem_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "cem", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-only", "--std", *[repr(float(v)) for v in std]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"profile": "no kernel_stats.csv"}
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            avg = float(row.get("AverageNs", row.get("AverageNS", "nan")))
            calls = int(row.get("Calls", 0))
            for key, pat in (("update", "cem_update_kernel"), ("sample", "cem_sample_kernel"), ("rollout", "rollout_kernel")):
                if pat in name and f"{key}_us" not in out:
                    out[f"{key}_us"] = avg / 1e3
                    out[f"{key}_calls"] = calls
    shutil.rmtree(d, ignore_errors=True)
    return out


def loop(lam, std, n_steps=500):
    mpc = rovmpc.MPC(N=N, K=K, device_sampling=True)
    rows, _ = closed_loop_inputs(mpc.engine, 12, n_steps)
    mppi = rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=1)
    cem = rovmpc.CEM(N=N, K=K, n_elite=E, std=std, n_iter=1)
    res = {}
    for name, c in (("shooting", mpc), ("mppi", mppi), ("cem", cem)):
        us, Js = [], []
        for r in rows:
            us.append(c.step(r).copy())
            Js.append(c.last.cost)
        us, Js = np.array(us), np.array(Js)
        fin = np.isfinite(Js)
        res[name] = {"mean_J_star": float(Js[fin].mean()) if fin.any() else float("nan"), "finite_steps": int(fin.sum()),
                     "sum_du": float(np.linalg.norm(np.diff(us, axis=0), axis=1).sum())}
    mpc.close(); mppi.close(); cem.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--std", type=float, nargs=3, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    model = rovmpc.default_model()
    std = np.asarray(a.std if a.std else model.scale[3:6], dtype=np.float64)
    state, _ = rovmpc.synthetic_problem(1, N)
    if a.kernel_only:
        kernel_only(std, state)
        return
    lam = pick_lambda(state, std)
    out = {"N": N, "K": K, "n_elite": E, "dtype": "f64", "lambda": lam, "steps": a.steps}
    out.update(time_steps(max(a.steps, 500), lam, std, state))
    out["cem_I1_over_mppi_I1"] = out["cem_I1_us"] / out["mppi_I1_us"]
    print(f"rovmpc_mpc_step_sampled          : {out['mpc_step_sampled_us']:8.2f} us/step")
    print(f"rovmpc_mppi_step, n_iter = 1     : {out['mppi_I1_us']:8.2f} us/step")
    for I in (1, 2, 4):
        print(f"rovmpc_cem_step, n_iter = {I}      : {out[f'cem_I{I}_us']:8.2f} us/step")
    print(f"CEM (I = 1) / MPPI (I = 1)       : {out['cem_I1_over_mppi_I1']:8.2f}x")
    if not a.no_profile:
        p = profile(std)
        out["kernels"] = p
        if "update_us" in p:
            print(f"cem_update_kernel                : {p['update_us']:8.2f} us")
            print(f"cem_sample_kernel                : {p.get('sample_us', float('nan')):8.2f} us")
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
