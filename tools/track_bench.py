#!/usr/bin/env python3
"""The marker tracker (rovmpc_track_markers_device) against what the library could already do: a chain of stream-ordered
rovmpc_fit_theta_gamma_device launches whose d_guess is the previous frame's out row.  M = 16, L = 3 m, ENU, bracket (1e-6, 200): with the default c_hi = 10
a sixth of these frames is the chord at the truth (the root of the rotated system lies beyond it).

Recordings: B cables of T = 2048 frames around the vehicle of rovmpc.synthetic_problem, the vehicle drifting slowly, (theta,
gamma) smooth sinusoids, markers from rovmpc_transform_catenary; no dropouts, and both chains enter frame 0 from the truth
there (the tracker as its incoming carry), so both give the same angles (checked).
The handle's stream is its own, so the fit chain cannot put a strided copy between its launches: a launch takes its guess
[B'][2] from one place, and only for B' = 1 is that the previous out row.  The chain for B recordings is therefore B T
launches of one frame, frame-major (all recordings' frame t before any frame t + 1).  No status can redirect it.

1. Wall time per recording set (enqueue to synchronise) of the fit chain and of one tracker call, alternating, for B = 1 and
   B = 64; mean trial steps per frame of each.
2. Device time: the kernels' durations summed from a separate `rocprofv3 --kernel-trace` run of this script (--kernel-only).
3. The 4096 frames of tools/fit_bench.py as 4096 one-frame recordings with the default start list: how many of the frames
   that answer CHORD from (0, 0) are ACQUIRED.
4. `make resource-usage` lines of the two kernels (compiled here with hipcc, no GPU needed).

Usage: python tools/track_bench.py [--reps 3] [--no-profile] [--json OUT]
"""
import argparse
import csv
import ctypes as C
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
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import rovmpc  # noqa: E402

M, T = 16, 2048
BS = (1, 64)
C_HI = 200.0
_engine = None


def bench_engine():
    global _engine
    if _engine is None:
        _engine = rovmpc.Engine(rovmpc.MPCConfig(N=1, K=1, c_hi=C_HI))
    return _engine


def recordings(B, seed=11):
    """(P0, P1 (B, T, 3), Y (B, T, M, 3), truth (B, T, 2)), every frame a catenary."""
    rng = np.random.default_rng(seed)
    e = bench_engine()
    state, _ = rovmpc.synthetic_problem(1, 1)
    t = np.arange(T)
    ph = rng.uniform(0, 2 * np.pi, (B, 4))
    P1 = state[3:6] + 0.1 * np.stack([np.sin(0.004 * t + ph[:, 0:1]), np.cos(0.003 * t + ph[:, 1:2]), 0.5 * np.sin(0.005 * t + ph[:, 2:3])], axis=-1)
    th = 0.25 * np.sin(0.01 * t + ph[:, 2:3])
    ga = 0.3 * np.cos(0.013 * t + ph[:, 3:4])
    out, npts, _ = e.transform_catenary(np.zeros((B * T, 3)), P1.reshape(-1, 3), th.ravel(), ga.ravel(), e.cfg.L, M)
    if not np.all(npts[:, 1] == M):
        raise SystemExit("a frame of the clean recording is the chord: change the seed")
    return np.zeros((B, T, 3)), np.ascontiguousarray(P1), np.ascontiguousarray(out[3].reshape(B, T, M, 3)), np.stack([th, ga], axis=-1)


class Runs:
    """Device buffers of one recording set and the two chains over them, each a callable that enqueues and synchronises."""

    def __init__(self, e, B):
        import torch
        self.e, self.B, self.torch = e, B, torch
        self.dev = torch.device("cuda", e.cfg.device)
        P0, P1, Y, self.truth = recordings(B)
        up = lambda x: torch.tensor(np.ascontiguousarray(x), device=self.dev)
        self.t0, self.t1, self.tY = up(P0), up(P1), up(Y)                                  # [B][T]...: the tracker's layout
        self.f0, self.f1, self.fY = up(P0.swapaxes(0, 1)), up(P1.swapaxes(0, 1)), up(Y.swapaxes(0, 1))     # [T][B]...: the chain's
        self.t_out = torch.zeros((B, T, 9), dtype=torch.float64, device=self.dev)
        self.f_out = torch.zeros((T, B, 6), dtype=torch.float64, device=self.dev)
        self.c0 = up(self.truth[:, 0])                                                      # [B][2]: where both chains start
        self.tc = torch.zeros_like(self.c0)
        self.tp = rovmpc.TrackParams.make()
        self.fp = rovmpc.FitParams.make()
        lib, h = e.lib, e._h
        fit = lib.rovmpc_fit_theta_gamma_device
        p0, p1, pY, po, pc = (x.data_ptr() for x in (self.f0, self.f1, self.fY, self.f_out, self.c0))
        fpr = C.byref(self.fp)
        # frame-major one-frame launches; the guess of (t, b) is the out row of (t - 1, b), the common start at t = 0
        self.fit_calls = [(h, p0 + 24 * i, p1 + 24 * i, pY + 24 * M * i, 1, M, (po + 48 * (i - B)) if i >= B else pc + 16 * i, fpr, po + 48 * i)
                          for i in range(T * B)]
        self.fit = fit
        torch.cuda.synchronize(self.dev)

    def fit_chain(self):
        """Wall milliseconds from the first enqueue to the synchronise."""
        fit = self.fit
        t0 = time.perf_counter()
        for a in self.fit_calls:
            fit(*a)
        self.torch.cuda.synchronize(self.dev)
        return (time.perf_counter() - t0) * 1e3

    def tracker(self):
        self.tc.copy_(self.c0)                                                              # (the call writes the carry back)
        self.torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        rc = self.e.lib.rovmpc_track_markers_device(self.e._h, self.t0.data_ptr(), self.t1.data_ptr(), self.tY.data_ptr(), self.B, T, M,
                                                    self.tc.data_ptr(), C.byref(self.tp), self.t_out.data_ptr(), None)
        self.torch.cuda.synchronize(self.dev)
        assert rc == 0
        return (time.perf_counter() - t0) * 1e3


def compare(reps):
    e = bench_engine()
    res = {}
    for B in BS:
        r = Runs(e, B)
        r.fit_chain(); r.tracker()                                                           # warm-up, and the results to compare
        f, t = r.f_out.cpu().numpy().swapaxes(0, 1), r.t_out.cpu().numpy()
        tag = f"B{B}"
        res[f"{tag}_same_angle_bits"] = bool(np.array_equal(f[..., 0:2], t[..., 0:2]))
        res[f"{tag}_max_angle_difference_rad"] = float(np.abs(f[..., 0:2] - t[..., 0:2]).max())
        res[f"{tag}_max_angle_error_rad"] = float(np.abs(t[..., 0:2] - r.truth).max())
        res[f"{tag}_fit_chain_all_converged"] = bool(np.all(f[..., 5] == 0))
        res[f"{tag}_tracker_states"] = {s.name: int((t[..., 7] == s).sum()) for s in rovmpc.TrackState if (t[..., 7] == s).any()}
        res[f"{tag}_fit_chain_mean_trial_steps"] = float(f[..., 4].mean())
        res[f"{tag}_tracker_mean_trial_steps"] = float(t[..., 5].mean())
        res[f"{tag}_tracker_mean_trial_steps_locked"] = float(t[..., 5][t[..., 7] == 0].mean())
        wf, wt = [], []
        for _ in range(reps):                                                                # alternating
            wf.append(r.fit_chain()); wt.append(r.tracker())
        res[f"{tag}_fit_chain_wall_ms"] = wf
        res[f"{tag}_tracker_wall_ms"] = wt
        res[f"{tag}_fit_chain_launches"] = len(r.fit_calls)
        res[f"{tag}_tracker_launches"] = -(-T // 256)
    return res


def acquisition():
    """tools/fit_bench.py's 4096 frames, cold and as one-frame recordings."""
    import fit_bench
    e = rovmpc.default_engine()
    res = {}
    for noise, tag in ((0.0, "noise_free"), (1e-3, "noisy")):
        P0, P1, Y, truth = fit_bench.frames(4096, noise)
        cold = e.fit_theta_gamma(P0, P1, Y)
        chord = cold.status == rovmpc.FitStatus.CHORD
        tr = e.track_markers(P0[:, None], P1[:, None], Y[:, None])
        state = tr.state[:, 0]
        acq = state == rovmpc.TrackState.ACQUIRED
        err = np.abs(np.stack([tr.theta[:, 0], tr.gamma[:, 0]], axis=1) - truth)
        res[tag] = {"cold_chord": int(chord.sum()), "cold_chord_acquired": int((chord & acq).sum()),
                    "tracker_states": {s.name: int((state == s).sum()) for s in rovmpc.TrackState if (state == s).any()},
                    "acquired_start_index_counts": {int(k): int((tr.start[:, 0][acq] == k).sum()) for k in np.unique(tr.start[:, 0][acq])},
                    "cold_chord_acquired_within_1e-9_rad_of_truth": int((chord & acq & (err.max(axis=1) < 1e-9)).sum()),
                    "cold_chord_acquired_max_angle_error_rad": float(err[chord & acq].max()) if (chord & acq).any() else None}
    return res


def kernel_only():
    e = bench_engine()
    for B in BS:
        r = Runs(e, B)
        r.fit_chain(); r.tracker()


def profile():
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"profile": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="track_prof_")
    cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "track", "--", sys.executable, os.path.abspath(__file__), "--kernel-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        return {"profile": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return {"profile": "no kernel_trace.csv"}
    rows = {"fit_theta_gamma_kernel": [], "track_markers_kernel": []}
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            for k in rows:
                if k in row["Kernel_Name"]:
                    rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {k + "_dispatches": len(v) for k, v in rows.items()}
    fit, trk = sorted(rows["fit_theta_gamma_kernel"]), sorted(rows["track_markers_kernel"])
    nl = -(-T // 256)
    if len(fit) == T * sum(BS) and len(trk) == nl * len(BS):
        lo_f = lo_t = 0
        for B in BS:
            part_f, part_t = fit[lo_f:lo_f + T * B], trk[lo_t:lo_t + nl]
            lo_f += T * B; lo_t += nl
            out[f"B{B}_fit_chain_device_ms"] = sum(b - a for a, b in part_f) / 1e6
            out[f"B{B}_fit_chain_first_to_last_ms"] = (part_f[-1][1] - part_f[0][0]) / 1e6
            out[f"B{B}_tracker_device_ms"] = sum(b - a for a, b in part_t) / 1e6
            out[f"B{B}_tracker_device_us_per_frame"] = out[f"B{B}_tracker_device_ms"] * 1e3 / T
            out[f"B{B}_fit_kernel_us_per_launch"] = out[f"B{B}_fit_chain_device_ms"] * 1e3 / (T * B)
    shutil.rmtree(d, ignore_errors=True)
    return out


def resource_usage():
    """The -Rpass-analysis=kernel-resource-usage remarks of the two kernels in helpers_host.hip."""
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
            name = next((k for k in ("fit_theta_gamma_kernel", "track_markers_kernel") if k in m.group(2)), None)
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
    ap.add_argument("--resource-usage-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.kernel_only:
        kernel_only()
        return
    if a.resource_usage_only:
        out = {"resource_usage": resource_usage()}
    else:
        out = {"M": M, "T": T, "track_chunk": 256, "L": rovmpc.MPCConfig().L, "bracket": [rovmpc.MPCConfig().c_lo, C_HI]}
        out.update(compare(a.reps))
        out["fit_bench_frames_as_one_frame_recordings"] = acquisition()
        if not a.no_profile:
            out["kernels"] = profile()
        out["resource_usage"] = resource_usage()
    for k, v in out.items():
        print(f"{k:44s} : {v}")
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
