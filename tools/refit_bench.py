#!/usr/bin/env python3
"""Time rovmpc_refit_rows: the 37 generation-1 rows refitted, pooled, on B = 1 and B = 8 recordings of 2048 rows.

Per B it reports the host entry (uploads, launch, synchronise), the device entry with the recordings resident (enqueue and
synchronise: the kernel plus one launch), and scipy.optimize.least_squares (method "lm", finite-difference Jacobian, NumPy
residuals) on the same problems on the CPU.  The device time of refit_rows_kernel itself comes from a separate
`rocprofv3 --kernel-trace` run of this file (--kernel-only: one host call per B).  Nothing is asserted; the figures go to
profiles/refit_bench.json.

    python tools/refit_bench.py [--reps 5] [--no-profile] [--out profiles/refit_bench.json]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rovmpc  # noqa: E402
from rovmpc import _lib  # noqa: E402
from rovmpc.engine import _ptr  # noqa: E402
from rovmpc.expr import OP, compile_expression  # noqa: E402
from rovmpc.scoring import default_free  # noqa: E402

T = 2048


def workload(B):
    """Rows, X (B, T, 18), target (B, T): the recorded table tiled to 2048 rows with 1 % jitter; the target is the chosen theta
    row on it plus 1e-3 std noise."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "kat_replay.npz"))
    eqs = json.load(open(os.path.join(ROOT, "tests", "golden", "equations.json")))
    rows = [r["sympy_format"] for key in ("dtheta_dt", "dgamma_dt") for r in eqs[key]["rows"]]
    rng = np.random.default_rng(2048 + B)
    base = np.asarray(d["Xs"], dtype=np.float64)
    X = np.stack([np.tile(base, (T // len(base) + 1, 1))[:T] * (1 + 0.01 * rng.standard_normal((T, base.shape[1]))) for _ in range(B)])
    front = eqs["dtheta_dt"]
    chosen = [r for r in front["rows"] if r["complexity"] == front["chosen_complexity"]][0]["sympy_format"]
    clean = np.stack([values(chosen, x) for x in X])
    return rows, X, clean + 1e-3 * clean.std() * rng.standard_normal(clean.shape)


def run_code(code, consts, X):
    """The bytecode on the rows of X in NumPy."""
    st = []
    un = {OP["NEG"]: np.negative, OP["SIN"]: np.sin, OP["COS"]: np.cos, OP["TANH"]: np.tanh, OP["ABS"]: np.abs, OP["SQUARE"]: np.square,
          OP["EXP"]: np.exp, OP["LOG"]: np.log, OP["SQRT"]: np.sqrt, OP["SAFE_LOG"]: lambda a: np.log(np.abs(a) + 1e-5),
          OP["SAFE_SQRT"]: lambda a: np.sqrt(np.abs(a))}
    bi = {OP["ADD"]: np.add, OP["SUB"]: np.subtract, OP["MUL"]: np.multiply, OP["DIV"]: np.divide, OP["POW"]: np.power}
    with np.errstate(all="ignore"):
        for ins in code:
            op, arg = ins & 0xFF, ins >> 8
            if op == OP["PUSH_C"]:
                st.append(np.full(len(X), consts[arg]))
            elif op == OP["PUSH_F"]:
                st.append(X[:, arg])
            elif op in bi:
                b = st.pop(); st[-1] = bi[op](st[-1], b)
            elif op == OP["POWI"]:
                st[-1] = st[-1] ** float(arg - (1 << 24) if arg >= (1 << 23) else arg)
            else:
                st[-1] = un[op](st[-1])
    return st[0]


def values(text, X):
    consts = []
    return run_code(compile_expression(text, consts, X.shape[1]).code, consts, X)


def scipy_fits(rows, X, target):
    from scipy.optimize import least_squares
    Xf, g = X.reshape(-1, X.shape[-1]), target.reshape(-1)
    t0 = time.perf_counter()
    losses = []
    for text in rows:
        consts = []
        code = compile_expression(text, consts, Xf.shape[1]).code
        c0 = np.array(consts, dtype=np.float64)
        free = np.flatnonzero(default_free(code, len(consts), text))
        if len(free) == 0:
            losses.append(float(np.mean((run_code(code, c0, Xf) - g) ** 2)))
            continue

        def res(p):
            c = c0.copy(); c[free] = p
            return np.nan_to_num(run_code(code, c, Xf) - g, nan=1e6, posinf=1e6, neginf=-1e6)
        sol = least_squares(res, c0[free], method="lm", xtol=1e-12, ftol=1e-15, gtol=1e-10, max_nfev=50 * (len(free) + 1))
        losses.append(float(2 * sol.cost / len(g)))
    return (time.perf_counter() - t0) * 1e3, losses


BS = (1, 8)


def kernel_only():
    for B in BS:
        rovmpc.refit_rows(*workload(B))


def profile():
    """{B: device time of refit_rows_kernel in ms} from a `rocprofv3 --kernel-trace` run of kernel_only(), or why not."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="refit_prof_")
    cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "refit", "--", sys.executable, os.path.abspath(__file__), "--kernel-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv"}
    with open(traces[0]) as f:
        spans = sorted((int(row["Start_Timestamp"]), int(row["End_Timestamp"])) for row in csv.DictReader(f) if "refit_rows_kernel" in row["Kernel_Name"])
    if len(spans) != len(BS):
        return {"profile": f"{len(spans)} refit_rows_kernel dispatches, expected {len(BS)}"}
    return {B: (e - s) / 1e6 for B, (s, e) in zip(BS, spans)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_bench.json"))
    a = ap.parse_args()
    if a.kernel_only:
        kernel_only()
        return
    kernel_ms = {"profile": "skipped"} if a.no_profile else profile()      # (the child runs before this process opens the GPU)
    import torch
    eng = rovmpc.default_engine()
    dev = torch.device("cuda", eng.cfg.device)
    results = []
    for B in BS:
        rows, X, target = workload(B)
        fit = rovmpc.refit_rows(rows, X, target)                                         # warm-up, and the figures of the fits
        host = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); rovmpc.refit_rows(rows, X, target); host.append((time.perf_counter() - t0) * 1e3)
        # the device entry on resident buffers, bound by hand so that nothing but the call is timed
        progs, masks = [], []
        for text in rows:
            consts = []
            code = compile_expression(text, consts, X.shape[2]).code
            progs.append((code, consts)); masks.append(default_free(code, len(consts), text))
        code = np.concatenate([np.asarray(c, np.int32) for c, _ in progs]).astype(np.int32)
        consts = np.concatenate([np.asarray(k, np.float64) for _, k in progs] + [np.zeros(1)])
        mask = np.concatenate([m for m in masks] + [np.zeros(1, np.uint8)]).astype(np.uint8)
        code_off = np.cumsum([0] + [len(c) for c, _ in progs]).astype(np.int32)
        const_off = np.cumsum([0] + [len(k) for _, k in progs]).astype(np.int32)
        dX, dG = torch.tensor(X, device=dev), torch.tensor(target, device=dev)
        dK = torch.empty(max(int(const_off[-1]), 1), dtype=torch.float64, device=dev)
        dO = torch.empty((len(rows), 1, _lib.REFIT_OUT), dtype=torch.float64, device=dev)
        params = _lib.RefitParams.make()
        device = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng._check(eng.lib.rovmpc_refit_rows_device(eng._h, _ptr(code), _ptr(code_off), _ptr(consts), _ptr(const_off), _ptr(mask), len(rows),
                                                        dX.data_ptr(), X.shape[2], None, T, B, dG.data_ptr(), None, 1, C.byref(params),
                                                        dK.data_ptr(), dO.data_ptr()))
            torch.cuda.synchronize(dev)
            device.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(dO.cpu().numpy()[:, 0, 1], fit.loss[:, 0], equal_nan=True)
        cpu_ms, cpu_loss = scipy_fits(rows, X, target)
        names = [rovmpc.RefitStatus(int(s)).name for s in fit.status[:, 0]]
        results.append(dict(B=B, T=T, rows=len(rows), host_call_ms=dict(min=min(host), median=float(np.median(host))),
                            device_call_ms=dict(min=min(device[1:]), median=float(np.median(device[1:]))),
                            refit_rows_kernel_ms=kernel_ms.get(B, kernel_ms.get("profile")), scipy_least_squares_ms=cpu_ms, status={n: names.count(n) for n in sorted(set(names))},
                            trial_steps=dict(total=int(fit.iters.sum()), max=int(fit.iters.max())),
                            rows_below_scipy_loss=int(np.sum(fit.loss[:, 0] <= np.array(cpu_loss) * (1 + 1e-9))),
                            median_loss=float(np.nanmedian(fit.loss)), median_scipy_loss=float(np.nanmedian(cpu_loss))))
        print(json.dumps(results[-1]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(dict(tool="tools/refit_bench.py", device=torch.cuda.get_device_name(dev), reps=a.reps, results=results), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
