#!/usr/bin/env python3
"""The navigation cost of MPPI and CEM (rovmpc_set_nav_cost) at C2 (N = 20, K = 4096, fp64, n_iter = 1).

1. Host-clock microseconds per control step (one prepared ctypes call each, >= 500 steps after warm-up) of rovmpc_mppi_step
   and rovmpc_cem_step without and with a navigation cost (a 64-row track, all four terms, 2 spheres), in one process.
2. nav_cost_kernel's device time next to mppi_sample_kernel (the kernel that writes the 2 MB this one reads) and the other
   kernels of the step, from a separate `rocprofv3 --kernel-trace --stats` run of this script (--kernel-only): 300 MPPI
   steps with the cost on.  --stats-csv keeps the trace's kernel_stats.csv.
3. A 500-step loop over the measured rows of Rov_traj_gen case 12 (closed_loop_inputs), MPPI and CEM, without a navigation
   cost and with a rate term alone (w_du on every channel): mean J* and sum |u_t - u_{t-1}|.  Reported, not asserted.

Usage: python tools/nav_bench.py [--steps 2000] [--no-profile] [--json OUT] [--stats-csv OUT] [--w-du 1e-6 1e-5]
"""
import argparse
import ctypes as C
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rovmpc  # noqa: E402
from rovmpc._lib import State  # noqa: E402
from rovmpc.closed_loop import closed_loop_inputs  # noqa: E402

N, K = 20, 4096
KERNELS = (("nav_cost", "nav_cost_kernel"), ("mppi_sample", "mppi_sample_kernel"), ("mppi_update", "mppi_update_kernel"),
           ("rollout", "rollout_kernel"))


def pick_lambda(state, std):
    """A temperature on the scale of the spread of the costs of one draw around the default nominal."""
    m = rovmpc.MPPI(N=N, K=K, lam=1.0, std=std, n_iter=1)
    m.step(state)
    _, J = m.engine.mppi_last()
    m.close()
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


def bench_nav(state):
    """All four terms: a 64-row track leaving the vehicle's position at the mean control, 2 spheres beside it."""
    m = rovmpc.default_model()
    c = 1e-3 / 60.0
    track = state[3:6] + c * m.mean[3:6] * np.arange(1, 65)[:, None]
    spheres = [list(track[10] + 0.01) + [0.02], list(track[40] - 0.01) + [0.02]]
    return rovmpc.NavCost(track, w_pos=1e3, w_term=1e4, w_du=1e-6, w_sphere=1e4, spheres=spheres)


def controller(kind, nav, lam, std):
    if kind == "mppi":
        return rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=1, nav=nav)
    return rovmpc.CEM(N=N, K=K, std=std, n_iter=1, nav=nav)


def time_steps(steps, lam, std, state):
    out = {}
    st = State()
    C.memmove(C.byref(st), np.ascontiguousarray(state, np.float64).ctypes.data, 128)
    for kind in ("mppi", "cem"):
        for setting, nav in (("plain", None), ("nav", bench_nav(state))):
            ctl = controller(kind, nav, lam, std)
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
    return out


def kernel_only(lam, std, state, steps=300):
    ctl = controller("mppi", bench_nav(state), lam, std)
    for _ in range(steps):
        ctl.step(state)
    ctl.close()


def profile(lam, std, stats_csv):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="nav_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "nav", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-only", "--lam", repr(lam), "--std", *[repr(float(v)) for v in std]]
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
            for key, pat in KERNELS:
                # the kernel's own name, or its specialised forms (rollout_kernel_lean16_n20); not another kernel's
                if re.search(rf"\b{pat}\w*<", name) and f"{key}_us" not in out:
                    out[f"{key}_us"] = avg / 1e3
                    out[f"{key}_calls"] = int(row.get("Calls", 0))
    if stats_csv:
        os.makedirs(os.path.dirname(os.path.abspath(stats_csv)), exist_ok=True)
        shutil.copyfile(files[0], stats_csv)
    shutil.rmtree(d, ignore_errors=True)
    if "nav_cost_us" in out and "mppi_sample_us" in out:
        out["nav_over_mppi_sample"] = out["nav_cost_us"] / out["mppi_sample_us"]
    return out


def loop(lam, std, w_dus, n_steps=500):
    res = {}
    for kind in ("mppi", "cem"):
        for w_du in (0.0,) + tuple(w_dus):
            ctl = controller(kind, None, lam, std)
            rows, _ = closed_loop_inputs(ctl.engine, 12, n_steps)
            if w_du:
                ctl.set_nav(rovmpc.NavCost(rows[:, 3:6], w_du=w_du))
            r = ctl.run(rows)
            Js, fin = r.cost, np.isfinite(r.cost)
            res[f"{kind}_w_du_{w_du:g}"] = {"mean_J_star": float(Js[fin].mean()) if fin.any() else float("nan"), "finite_steps": int(fin.sum()),
                                           "sum_du": float(np.linalg.norm(np.diff(r.u, axis=0), axis=1).sum())}
            ctl.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--lam", type=float, default=None)
    ap.add_argument("--std", type=float, nargs=3, default=None)
    ap.add_argument("--w-du", type=float, nargs="+", default=[1e-6, 1e-5])
    ap.add_argument("--json", default=None)
    ap.add_argument("--stats-csv", default=None)
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
    for kind in ("mppi", "cem"):
        for setting in ("plain", "nav"):
            print(f"rovmpc_{kind}_step, {setting:5s}          : {out[f'{kind}_{setting}_us']:8.2f} us/step")
    if not a.no_profile:
        p = profile(lam, std, a.stats_csv)
        out["kernels"] = p
        if "profile" in p:
            print("profile:", p)
        for key, pat in KERNELS:
            if f"{key}_us" in p:
                print(f"{pat:32s} : {p[f'{key}_us']:8.2f} us  ({p[f'{key}_calls']} calls)")
        if "nav_over_mppi_sample" in p:
            print(f"nav_cost_kernel / mppi_sample_kernel : {p['nav_over_mppi_sample']:.2f}x")
    out["loop_case12"] = loop(lam, std, a.w_du)
    for name, r in out["loop_case12"].items():
        print(f"case 12, 500 steps, {name:16s}: mean J* {r['mean_J_star']:.6g}, sum |du| {r['sum_du']:.6g}, "
              f"finite steps {r['finite_steps']}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
