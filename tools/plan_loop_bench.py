#!/usr/bin/env python3
"""Device-resident MPPI / CEM closed loops at C2 (N = 20, K = 4096, fp64, E = 64) against the host-stepped loop.

Protocol of DESIGN.md section 8c: the parent's library and this one side by side (--parent LIB), runs interleaved
(parent, new, parent, new, ...), one process per run (--turns of each), a host clock over --steps control steps.

1. us per control step (and per problem) of the host-stepped loop -- one blocking rovmpc_*_step / _step_batch per step over
   the rows of closed_loop_inputs(engine, 12, steps) -- on the parent's library and on this one, and of ONE
   rovmpc_*_closed_loop[_batch]_device call over the same rows on this one; MPPI and CEM, n_iter 1 and 2, B = 1, 8, 64.
   Accepted when the device loop's mean lies below the parent's host-stepped mean by more than the parent's min-max spread.
2. The single steps (the B = 1 host-stepped figures) of this library against the parent's: not slower by more than the
   parent's spread.
3. Launches per control step and the update kernels' time with and without the hand-off, from two
   `rocprofv3 --kernel-trace --stats` runs of this script of their own (--kernel-only loop / step).
4. Case 12, 500 steps, feedback 0 and 1: mean J* and sum |u_t - u_{t-1}| of the device loop (feedback 0 also host-stepped).

Usage: python tools/plan_loop_bench.py --parent /path/to/parent/librovmpc.so [--turns 3] [--steps 2000] [--out-dir profiles]
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

N, K, E = 20, 4096, 64
BATCHES = (1, 8, 64)
ITERS = (1, 2)
KINDS = ("mppi", "cem")
P = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(P)


def controller(rovmpc, kind, B, I, lam, std):
    if B == 0:
        return rovmpc.MPPI(N=N, K=K, lam=lam, std=std, n_iter=I) if kind == "mppi" else rovmpc.CEM(N=N, K=K, n_elite=E, n_iter=I, std=std)
    if kind == "mppi":
        return rovmpc.BatchedMPPI(N=N, K=K, B=B, lam=lam, std=std, n_iter=I)
    return rovmpc.BatchedCEM(N=N, K=K, B=B, n_elite=E, n_iter=I, std=std)


def pick_lambda(rovmpc, std, state):
    m = rovmpc.MPPI(N=N, K=K, lam=1.0, std=std, n_iter=1)
    m.step(state)
    _, J = m.engine.mppi_last()
    m.close()
    J = J[np.isfinite(J)]
    return float(max(np.median(J - J.min()), 1e-12))


def rows_of(rovmpc, ctl, steps):
    from rovmpc.closed_loop import closed_loop_inputs
    return closed_loop_inputs(ctl.engine, 12, steps)[0]


def host_stepped(rovmpc, kind, B, I, lam, std, steps, warm=50):
    """us per control step of `steps` blocking step calls; B = 1 is the single-problem entry."""
    from rovmpc._lib import State
    ctl = controller(rovmpc, kind, 0 if B == 1 else B, I, lam, std)
    e = ctl.engine
    rows = rows_of(rovmpc, ctl, steps + warm)
    if B == 1:
        rec = np.empty(e.result_len)
        states = [C.cast(rows.ctypes.data + 128 * i, C.POINTER(State)) for i in range(len(rows))]
        fn = e.lib.rovmpc_mppi_step if kind == "mppi" else e.lib.rovmpc_cem_step
        tail = (None, None) if kind == "mppi" else (None, None, None, None)
        call = lambda s: fn(e._h, states[s], 7, s, C.byref(ctl.params), ptr(rec), *tail)                         # noqa: E731
    else:
        rec = np.empty((B, e.result_len))
        st = np.ascontiguousarray(np.repeat(rows[:, None, :], B, axis=1))                                         # (T, B, 16)
        states = [P(st.ctypes.data + 128 * B * i) for i in range(len(rows))]
        seeds = ctl.seeds
        fn = e.lib.rovmpc_mppi_step_batch if kind == "mppi" else e.lib.rovmpc_cem_step_batch
        tail = (None, None) if kind == "mppi" else (None, None, None, None)
        call = lambda s: fn(e._h, B, states[s], ptr(seeds), s, C.byref(ctl.params), ptr(rec), *tail)             # noqa: E731
    for s in range(warm):
        assert call(s) == 0
    t0 = time.perf_counter()
    for s in range(warm, warm + steps):
        call(s)
    us = (time.perf_counter() - t0) / steps * 1e6
    ctl.close()
    return us


def device_loop(rovmpc, kind, B, I, lam, std, steps, warm=50):
    """us per control step of one rovmpc_*_closed_loop[_batch]_device call of `steps` steps (after one of `warm`)."""
    import torch
    ctl = controller(rovmpc, kind, 0 if B == 1 else B, I, lam, std)
    e = ctl.engine
    rows = rows_of(rovmpc, ctl, steps + warm)
    W = e.mppi_row_len() if kind == "mppi" else e.cem_row_len(E)
    if B == 1:
        exo = torch.tensor(rows, device="cuda")
        out = torch.empty((steps, W), dtype=torch.float64, device="cuda")
        fn = e.mppi_closed_loop_device if kind == "mppi" else e.cem_closed_loop_device
        call = lambda t0, n: fn(exo.data_ptr() + 128 * t0, n, False, 7, t0, ctl.params, out.data_ptr())          # noqa: E731
        call(0, warm)
    else:
        # [B][T][16]: the warm-up and the timed stretch are separate tensors (a problem's rows are contiguous)
        exo_w = torch.tensor(np.ascontiguousarray(np.broadcast_to(rows[:warm], (B, warm, 16))), device="cuda")
        exo_t = torch.tensor(np.ascontiguousarray(np.broadcast_to(rows[warm:], (B, steps, 16))), device="cuda")
        out = torch.empty((steps, B, W), dtype=torch.float64, device="cuda")
        fn = e.mppi_closed_loop_batch_device if kind == "mppi" else e.cem_closed_loop_batch_device
        call = lambda t0, n: fn((exo_w if t0 == 0 else exo_t).data_ptr(), n, False, ctl.seeds, t0, ctl.params, out.data_ptr())   # noqa: E731
        call(0, warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(warm, steps)
    us = (time.perf_counter() - t0) / steps * 1e6
    ctl.close()
    return us


def worker(a):
    """One process, one library (ROVMPC_LIB): every host-stepped figure, and with --device the device loops too."""
    import rovmpc
    std = np.asarray(rovmpc.default_model().scale[3:6], dtype=np.float64)
    out = {"lib": "parent" if os.environ.get("ROVMPC_LIB") else "in-tree", "host": {}, "device": {}}
    for kind in KINDS:
        for I in ITERS:
            for B in BATCHES:
                n = a.steps if B < 64 else max(a.steps // 4, 300)
                key = f"{kind}_I{I}_B{B}"
                out["host"][key] = host_stepped(rovmpc, kind, B, I, a.lam, std, n)
                if a.device:
                    out["device"][key] = device_loop(rovmpc, kind, B, I, a.lam, std, n)
    print("RESULT " + json.dumps(out))


def kernel_only(a):
    """For rocprofv3: `loop` = one device loop of 200 steps per controller, `step` = 200 host steps (n_iter 1 and 2)."""
    import rovmpc
    import torch
    std = np.asarray(rovmpc.default_model().scale[3:6], dtype=np.float64)
    for kind in KINDS:
        for I in ITERS:
            ctl = controller(rovmpc, kind, 0, I, a.lam, std)
            rows = rows_of(rovmpc, ctl, 200)
            if a.kernel_only == "loop":
                ctl.run(rows, True)
            else:
                for r in rows:
                    ctl.step(r)
            torch.cuda.synchronize()
            ctl.close()


KERNELS = (("sample", "_sample_kernel"), ("update", "_update_kernel"), ("rollout", "rollout_kernel"))


def profile(mode, lam, out_csv=None):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="plan_loop_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "plan_loop", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-only", mode, "--lam", repr(lam)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"profile": "no kernel_stats.csv"}
    if out_csv:
        shutil.copy(files[0], out_csv)
    # the controllers' launches by kernel name; every other kernel of the process (torch's fills and copies, a plant or
    # copy kernel if the library launched one) is listed on its own
    out = {"mode": mode, "kernels": [], "other_kernels": [], "launches": {k: 0 for k, _ in KERNELS}, "other_launches": 0}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name, calls = row.get("Name", ""), int(row.get("Calls", 0))
            avg = float(row.get("AverageNs", row.get("AverageNS", "nan"))) / 1e3
            kind = next((k for k, pat in KERNELS if pat in name), None)
            entry = {"name": name[:100], "calls": calls, "avg_us": avg}
            if kind:
                out["kernels"].append(dict(entry, kind=kind))
                out["launches"][kind] += calls
            else:
                out["other_kernels"].append(entry)
                out["other_launches"] += calls
    # 200 steps of each controller at n_iter 1 and 2: per kind 2 controllers x 200 x (1 + 2) launches
    out["control_steps"] = 2 * 200 * 2
    out["launches_expected_per_kind"] = 2 * 200 * 3
    shutil.rmtree(d, ignore_errors=True)
    return out


def case12(lam, steps=500):
    """mean J* and sum |u_t - u_{t-1}| of the loop over Rov_traj_gen case 12."""
    import rovmpc
    from rovmpc.closed_loop import run_plan_closed_loop
    std = np.asarray(rovmpc.default_model().scale[3:6], dtype=np.float64)
    out = {}
    for kind in KINDS:
        for fb in (0, 1):
            ctl = controller(rovmpc, kind, 0, 1, lam, std)
            rep = run_plan_closed_loop(ctl, 12, steps, feedback=bool(fb))
            fin = np.isfinite(rep.cost)
            out[f"{kind}_fb{fb}"] = {"mean_J": float(rep.cost[fin].mean()) if fin.any() else float("nan"), "finite_steps": int(fin.sum()),
                                      "sum_du": float(np.linalg.norm(np.diff(rep.u, axis=0), axis=1).sum()),
                                      "us_per_step_with_transfers": rep.wall_s / steps * 1e6}
            ctl.close()
            if fb == 0:                                    # host-stepped over the same rows: the same figures by construction
                ref = controller(rovmpc, kind, 0, 1, lam, std)
                rows = rows_of(rovmpc, ref, steps)
                u, J = [], []
                for r in rows:
                    u.append(ref.step(r).copy()); J.append(ref.last.cost)
                u, J = np.stack(u), np.asarray(J)
                out[f"{kind}_fb0_host"] = {"mean_J": float(J[np.isfinite(J)].mean()), "sum_du": float(np.linalg.norm(np.diff(u, axis=0), axis=1).sum()),
                                           "equal_bits": bool(np.array_equal(u.view(np.uint64), rep.u.view(np.uint64)))}
                ref.close()
    return out


def stat(v):
    return {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's librovmpc.so")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--lam", type=float, default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--kernel-only", default=None, choices=("loop", "step"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.kernel_only:
        return kernel_only(a)
    import rovmpc
    std = np.asarray(rovmpc.default_model().scale[3:6], dtype=np.float64)
    if a.lam is None:
        a.lam = pick_lambda(rovmpc, std, rovmpc.synthetic_problem(1, N)[0])
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def run_worker(lib):
        env = dict(os.environ)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(a.steps), "--lam", repr(a.lam)]
        if lib:
            env["ROVMPC_LIB"], env["ROVMPC_LIB_OLD_ABI"] = lib, "1"
        else:
            env.pop("ROVMPC_LIB", None)
            cmd.append("--device")
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"worker failed ({r.returncode}): {r.stderr[-2000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    runs = {"parent": [], "new": []}
    for t in range(a.turns):
        if a.parent:
            runs["parent"].append(run_worker(a.parent))
        runs["new"].append(run_worker(None))
        say(f"turn {t + 1}/{a.turns} done")
    out = {"N": N, "K": K, "n_elite": E, "dtype": "f64", "lambda": a.lam, "steps": a.steps, "turns": a.turns, "loops": {}, "runs": runs}
    say(f"C2: N = {N}, K = {K}, fp64, n_elite = {E}, lambda = {a.lam:.6g}; {a.steps} steps (B = 64: {max(a.steps // 4, 300)}), {a.turns} processes per library, interleaved")
    say("us per control step (mean [min, max] over the processes); per problem in brackets for B > 1")
    say(f"{'':14s}{'parent host-stepped':>26s} {'new host-stepped':>26s} {'new device loop':>26s}  {'gain':>7s} {'spread':>7s}  loop  step")
    for kind in KINDS:
        for I in ITERS:
            for B in BATCHES:
                key = f"{kind}_I{I}_B{B}"
                new_h, dev = stat([r["host"][key] for r in runs["new"]]), stat([r["device"][key] for r in runs["new"]])
                par = stat([r["host"][key] for r in runs["parent"]]) if runs["parent"] else None
                row = {"parent_host": par, "new_host": new_h, "device": dev}
                fmt = lambda s: f"{s['mean']:8.2f} [{s['min']:7.2f},{s['max']:7.2f}]"                                   # noqa: E731
                if par:
                    spread = par["max"] - par["min"]
                    row["gain_us"], row["parent_spread_us"] = par["mean"] - dev["mean"], spread
                    row["loop_accepted"] = bool(par["mean"] - dev["mean"] > spread)
                    row["step_accepted"] = bool(new_h["mean"] - par["mean"] <= spread)
                    say(f"{key:14s}{fmt(par)} {fmt(new_h)} {fmt(dev)}  {row['gain_us']:7.2f} {spread:7.2f}  "
                        f"{'ok' if row['loop_accepted'] else 'MISS':>4s}  {'ok' if row['step_accepted'] else 'MISS':>4s}"
                        + (f"   per problem: {par['mean'] / B:.2f} -> {dev['mean'] / B:.2f}" if B > 1 else ""))
                else:
                    say(f"{key:14s}{'-':>26s} {fmt(new_h)} {fmt(dev)}")
                out["loops"][key] = row
    if not a.no_profile:
        os.makedirs(a.out_dir, exist_ok=True)
        out["profile"] = {m: profile(m, a.lam, os.path.join(a.out_dir, "plan_loop_kernel_stats.csv" if m == "loop" else "plan_loop_kernel_stats_step.csv"))
                          for m in ("loop", "step")}
        for m, p in out["profile"].items():
            if "kernels" not in p:
                say(f"profile {m}: {p}")
                continue
            say(f"rocprofv3, {m}: {p['control_steps']} control steps (200 per controller and n_iter 1, 2); launches sampler / rollout / update = "
                f"{p['launches']['sample']} / {p['launches']['rollout']} / {p['launches']['update']} (n_iter per step each would be "
                f"{p['launches_expected_per_kind']}); {p['other_launches']} launches of other kernels")
            for k in sorted(p["kernels"], key=lambda k: k["name"]):
                say(f"    {k['calls']:6d} x {k['avg_us']:8.2f} us  {k['name']}")
            for k in p["other_kernels"]:
                say(f"    other: {k['calls']:6d} x {k['avg_us']:8.2f} us  {k['name']}")
    out["case12"] = case12(a.lam)
    say("case 12, 500 steps, n_iter = 1 (device loop; fb0_host = the host-stepped loop over the same rows)")
    for k, v in out["case12"].items():
        say(f"    {k:14s} " + "  ".join(f"{n} = {x:.6g}" if isinstance(x, float) else f"{n} = {x}" for n, x in v.items()))
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "plan_loop_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out_dir, "plan_loop_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
