"""The calls whose bits tests/golden/fit_entries.npz records (tools/make_fit_golden.py writes it, tests/test_fit_golden_gpu.py
holds the library to it): rovmpc_fit_theta_gamma on every scene of fit_reference.scenes() from the scene's own start, and
from each start of the tracker's default list (STARTS), one host-entry call per (frame, M, max_iter) group."""
import numpy as np

import fit_reference as fr

STARTS = ((0.0, 0.0), (0.3, 0.0), (-0.3, 0.0), (0.6, 0.0), (-0.6, 0.0))


def engine(rv, up=1.0, dtype="f64"):
    return rv.Engine(rv.MPCConfig(N=1, K=1, dtype=dtype, c_lo=fr.BRACKET[0], c_hi=fr.BRACKET[1], L=fr.L_WS, frame="ENU" if up > 0 else "NED"))


def groups():
    g = {}
    for i, f in enumerate(fr.scenes()):
        g.setdefault((f.up, f.M, f.max_iter), []).append(i)
    return g


def rows_of(fit):
    return np.stack([np.asarray(c, dtype=np.float64) for c in fit], axis=1)


def run(rv, device=False):
    """{"own": (S, 6), "start0" .. "start4": (S, 6)} over the S scenes, by the host entry (or the device entry)."""
    S = len(fr.scenes())
    out = {"own": np.empty((S, fr.OUT))}
    out.update({f"start{k}": np.empty((S, fr.OUT)) for k in range(len(STARTS))})
    for (up, M, max_iter), idx in groups().items():
        fs = [fr.scenes()[i] for i in idx]
        A, P, Y = np.array([f.A for f in fs]), np.array([f.P for f in fs]), np.array([f.Y for f in fs])
        own = np.array([(0.0, 0.0) if f.guess is None else f.guess for f in fs])
        with engine(rv, up) as e:
            fit = e.fit_theta_gamma_device if device else e.fit_theta_gamma
            out["own"][idx] = rows_of(fit(A, P, Y, own, max_iter=max_iter))
            for k, s in enumerate(STARTS):
                out[f"start{k}"][idx] = rows_of(fit(A, P, Y, np.array(s), max_iter=max_iter))
    return out
