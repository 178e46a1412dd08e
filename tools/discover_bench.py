#!/usr/bin/env python3
"""Time rovmpc_discover_rows: the 55-term library {1, x_i, sin x_i, cos x_i} on B = 1 and B = 8 recordings of 2048 synthetic
scaled rows, pooled, max_terms = 8.

Per B it reports the host entry (uploads, two launches, synchronise), the device entry with the recordings resident (enqueue
and synchronise) and a NumPy baseline on the same machine: the terms evaluated per column, Phi^T Phi by one matrix product,
and the same greedy selection on that Gram (the reference restatement of stage 2 is not used: it is written for bits, not
speed; the baseline's selection is a vectorised Cholesky-style update).  GPU and NumPy runs alternate, three times each, and
the medians are reported.  The device times of discover_gram_kernel and discover_select_kernel come from a separate
`rocprofv3 --kernel-trace` run of this file (--kernel-only: one host call per B).  Nothing is asserted but that the two entries
agree to the bit (whether the baseline picks the same terms is recorded); the figures go to profiles/discover_bench.json.

    python tools/discover_bench.py [--reps 3] [--no-profile] [--out profiles/discover_bench.json]
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
from rovmpc.expr import compile_expression  # noqa: E402

T, F, S = 2048, 18, 8
BS = (1, 8)


def workload(B):
    """Terms, X (B, T, 18) N(0, 1), target (B, T): a four-term row of the library plus 1e-3 std noise."""
    rng = np.random.default_rng(4096 + B)
    X = rng.standard_normal((B, T, F))
    clean = 0.05 * (np.sin(X[..., 17]) - np.sin(X[..., 3]) - X[..., 16] - X[..., 3])
    return rovmpc.term_library(F), X, clean + 1e-3 * clean.std() * rng.standard_normal(clean.shape)


def numpy_discover(X, target, dep_tol=1e-10, min_gain=1e-12):
    """The baseline: columns, Gram, greedy forward selection.  Returns (picks, coefficients of the last size)."""
    Xf, g = X.reshape(-1, F), target.reshape(-1)
    Phi = np.concatenate([np.ones((len(Xf), 1)), Xf, np.sin(Xf), np.cos(Xf)], axis=1)
    G, b, c = Phi.T @ Phi, Phi.T @ g, float(g @ g)
    M = len(b)
    d = np.diag(G).copy()
    rho, q, W = d.copy(), b.copy(), np.zeros((S, M))
    free = np.ones(M, bool)
    picks, z = [], []
    for s in range(S):
        with np.errstate(all="ignore"):
            gain = np.where(free & (rho > dep_tol * d), q * q / rho, -np.inf)
        p = int(np.argmax(gain))
        if not gain[p] > min_gain * c:
            break
        l = np.sqrt(rho[p])
        w = (G[p] - W[:s].T @ W[:s, p]) / l
        w[p] = l
        W[s] = np.where(free, w, 0.0)
        z.append(q[p] / l)
        free[p] = False
        rho, q = rho - W[s] ** 2, q - W[s] * z[-1]
        picks.append(p)
    L = W[:len(picks)][:, picks].T
    return picks, np.linalg.solve(L.T, np.array(z)) if picks else np.zeros(0)


def kernel_only():
    for B in BS:
        terms, X, target = workload(B)
        rovmpc.discover_rows(terms, X, target, max_terms=S)


def profile():
    """{B: {kernel: device ms}} from a `rocprofv3 --kernel-trace` run of kernel_only(), or why not."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="discover_prof_")
    cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "discover", "--", sys.executable, os.path.abspath(__file__), "--kernel-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv"}
    out = {}
    with open(traces[0]) as f:
        rows = list(csv.DictReader(f))
    for name in ("discover_gram_kernel", "discover_select_kernel"):
        spans = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if name in r["Kernel_Name"])
        if len(spans) != len(BS):
            return {"profile": f"{len(spans)} {name} dispatches, expected {len(BS)}"}
        for B, (s, e) in zip(BS, spans):
            out.setdefault(B, {})[name + "_ms"] = (e - s) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discover_bench.json"))
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
        terms, X, target = workload(B)
        front = rovmpc.discover_rows(terms, X, target, max_terms=S)                      # warm-up, and the figures of the front
        progs = []
        for text in terms:
            consts = []
            progs.append((compile_expression(text, consts, F).code, consts))
        code = np.concatenate([np.asarray(c, np.int32) for c, _ in progs]).astype(np.int32)
        consts = np.concatenate([np.asarray(k, np.float64) for _, k in progs] + [np.zeros(1)])
        code_off = np.cumsum([0] + [len(c) for c, _ in progs]).astype(np.int32)
        const_off = np.cumsum([0] + [len(k) for _, k in progs]).astype(np.int32)
        dX, dG = torch.tensor(X, device=dev), torch.tensor(target, device=dev)
        dK = torch.empty((1, S), dtype=torch.int32, device=dev)
        dC = torch.empty((1, S, S), dtype=torch.float64, device=dev)
        dL = torch.empty((1, S + 1), dtype=torch.float64, device=dev)
        dI = torch.empty((1, 3), dtype=torch.int64, device=dev)
        params = _lib.DiscoverParams.make(S)

        def device_call():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng._check(eng.lib.rovmpc_discover_rows_device(eng._h, _ptr(code), _ptr(code_off), _ptr(consts), _ptr(const_off), len(terms),
                                                           dX.data_ptr(), F, None, T, B, dG.data_ptr(), None, 1, C.byref(params),
                                                           dK.data_ptr(), dC.data_ptr(), dL.data_ptr(), dI.data_ptr(), None))
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3
        device_call()                                                                    # warm-up
        host, device, cpu = [], [], []
        for _ in range(a.reps):                                                          # GPU and NumPy alternating
            t0 = time.perf_counter(); rovmpc.discover_rows(terms, X, target, max_terms=S); host.append((time.perf_counter() - t0) * 1e3)
            device.append(device_call())
            t0 = time.perf_counter(); picks, coef = numpy_discover(X, target); cpu.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(dC.cpu().numpy(), front.coef) and np.array_equal(dK.cpu().numpy(), front.picks)
        k = int(front.n_sel[0])
        results.append(dict(B=B, T=T, terms=len(terms), max_terms=S, n_sel=k, status=rovmpc.DiscoverStatus(int(front.status[0])).name,
                            picks=[terms[int(p)] for p in front.picks[0, :k]], loss=[float(v) for v in front.loss[0, :k + 1]],
                            host_call_ms=dict(min=min(host), median=float(np.median(host))),
                            device_call_ms=dict(min=min(device), median=float(np.median(device))),
                            numpy_ms=dict(min=min(cpu), median=float(np.median(cpu))),
                            kernels=kernel_ms.get(B, kernel_ms.get("profile")), numpy_picks_agree=picks == [int(p) for p in front.picks[0, :k]],
                            max_coef_diff_numpy=float(np.max(np.abs(coef - front.coef[0, len(picks) - 1, :len(picks)]))) if picks == [int(p) for p in front.picks[0, :k]] else None))
        print(json.dumps(results[-1]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(dict(tool="tools/discover_bench.py", device=torch.cuda.get_device_name(dev), reps=a.reps, results=results), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
