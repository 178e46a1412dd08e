#!/usr/bin/env python3
"""The shaped proposal of MPPI and CEM (time-correlated noise, MPPI box) at C2 (N = 20, K = 4096, fp64, n_iter = 1).

1. Host-clock microseconds per control step (one prepared ctypes call each, >= 500 steps after warm-up) of rovmpc_mppi_step
   and rovmpc_cem_step with white noise, with beta = 0.9 and with beta = 0.9 and a box, in one process.
2. The samplers' and the MPPI updates' device times from a separate `rocprofv3 --kernel-trace --stats` run of this script
   (--kernel-only), which steps all of those settings: the white samplers (mppi_sample_kernel, cem_sample_kernel) and the
   shaped one (proposal_sample_kernel) side by side in one trace, and mppi_update_kernel next to mppi_update_box_kernel.
   --stats-csv keeps the trace's kernel_stats.csv.
3. A 500-step loop over the measured rows of Rov_traj_gen case 12 (closed_loop_inputs) for beta = 0, 0.5, 0.9 on every
   channel: mean J* and sum |u_t - u_{t-1}| of MPPI and CEM.  Reported, not asserted.

Usage: python tools/proposal_bench.py [--steps 2000] [--no-profile] [--json OUT] [--stats-csv OUT]
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
SETTINGS = ("white", "beta", "beta_box")
KERNELS = (("mppi_sample", "mppi_sample_kernel"), ("cem_sample", "cem_sample_kernel"), ("proposal_sample", "proposal_sample_kernel"),
           ("mppi_update", "mppi_update_kernel"), ("mppi_update_box", "mppi_update_box_kernel"), ("cem_update", "cem_update_kernel"),
           ("rollout", "rollout_kernel"))


def pick_lambda(state, std):
    """A temperature on the scale of the spread of the costs of one draw around the default nominal."""
    m = rovmpc.MPPI(N=N, K=K, lam=1.0, std=std, n_iter=1)
    m.step(state)
    _, J = m.engine.mppi_last()
    m.close()
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


def box(std):
    mean = np.asarray(rovmpc.default_model().mean[3:6], dtype=np.float64)
    return mean - 2.0 * std, mean + 2.0 * std


def controller(kind, setting, lam, std, beta=0.9):
    """MPPI or CEM at C2 with one of SETTINGS (CEM's box is part of its parameters: the setting gives it a finite one)."""
    kw = {} if setting == "white" else {"beta": (beta,) * 3}
    if setting == "beta_box":
        kw["lo"], kw["hi"] = box(std)
    if kind == "mppi":
        return rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=1, **kw)
    return rovmpc.CEM(N=N, K=K, std=std, n_iter=1, **kw)


def time_steps(steps, lam, std, state):
    out = {}
    st = State()
    C.memmove(C.byref(st), np.ascontiguousarray(state, np.float64).ctypes.data, 128)
    for kind in ("mppi", "cem"):
        for setting in SETTINGS:
            ctl = controller(kind, setting, lam, std)
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
    for kind in ("mppi", "cem"):
        for setting in SETTINGS:
            ctl = controller(kind, setting, lam, std)
            for _ in range(steps):
                ctl.step(state)
            ctl.close()


def profile(lam, std, stats_csv):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="proposal_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "proposal", "--", sys.executable,
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
                # the kernel's own name (mppi_update_kernel is no prefix of mppi_update_box_kernel, nor of the batched forms)
                if f"{pat}<" in name and f"{key}_us" not in out:
                    out[f"{key}_us"] = avg / 1e3
                    out[f"{key}_calls"] = int(row.get("Calls", 0))
    if stats_csv:
        os.makedirs(os.path.dirname(os.path.abspath(stats_csv)), exist_ok=True)
        shutil.copyfile(files[0], stats_csv)
    shutil.rmtree(d, ignore_errors=True)
    for white in ("mppi_sample", "cem_sample"):
        if f"{white}_us" in out and "proposal_sample_us" in out:
            out[f"proposal_over_{white}"] = out["proposal_sample_us"] / out[f"{white}_us"]
    return out


def loop(lam, std, n_steps=500):
    res = {}
    for kind in ("mppi", "cem"):
        for beta in (0.0, 0.5, 0.9):
            ctl = controller(kind, "white" if beta == 0.0 else "beta", lam, std, beta)
            rows, _ = closed_loop_inputs(ctl.engine, 12, n_steps)
            r = ctl.run(rows)
            Js, fin = r.cost, np.isfinite(r.cost)
            res[f"{kind}_beta_{beta}"] = {"mean_J_star": float(Js[fin].mean()) if fin.any() else float("nan"), "finite_steps": int(fin.sum()),
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
        for setting in SETTINGS:
            print(f"rovmpc_{kind}_step, {setting:8s}       : {out[f'{kind}_{setting}_us']:8.2f} us/step")
    if not a.no_profile:
        p = profile(lam, std, a.stats_csv)
        out["kernels"] = p
        if "profile" in p:
            print("profile:", p)
        for key, pat in KERNELS:
            if f"{key}_us" in p:
                print(f"{pat:32s} : {p[f'{key}_us']:8.2f} us  ({p[f'{key}_calls']} calls)")
        for white in ("mppi_sample", "cem_sample"):
            if f"proposal_over_{white}" in p:
                print(f"proposal_sample_kernel / {white}_kernel : {p[f'proposal_over_{white}']:.2f}x")
    out["loop_case12"] = loop(lam, std)
    for name, r in out["loop_case12"].items():
        print(f"case 12, 500 steps, {name:14s}: mean J* {r['mean_J_star']:.6g}, sum |du| {r['sum_du']:.6g}, "
              f"finite steps {r['finite_steps']}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
