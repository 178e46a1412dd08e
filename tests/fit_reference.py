"""50-digit reference of the marker fit (law: include/rovmpc.h above rovmpc_fit_theta_gamma): the markers of a cable of known
(theta, gamma) from tests/tether_reference.py's node_points, the 50-digit minimiser and Jacobian, the plain fp64 NumPy
restatement `fit_np` of the header's iteration, the error scale that ties the tolerance to each frame's conditioning, and the
scenes both the host test and the GPU test run.

tests/test_fit_reference_host.py measures the margin M_FIT below on the CPU and checks the scenes' conditions;
tests/test_fit_gpu.py holds the kernel to the same bounds."""
import collections
import enum
import functools
import math

import numpy as np
from mpmath import mp, mpf

import cable_reference as cr
import tether_reference as tr

DPS = cr.DPS
EPS = cr.EPS
L_WS = cr.L_WS
BRACKET = tr.BRACKET

# the header's constants
H = 2.0 ** -20
MU0, MU_MIN = 1e-3, 1e-12
DET_MIN = 2.0 ** -80
SLACK = 2.0 ** -48
TOL, MAX_ITER = 1e-12, 40
OUT = 6


class Status(enum.IntEnum):
    CONVERGED = 0
    MAX_ITER = 1
    DEGENERATE = 2
    CHORD = 3
    TOO_FEW = 4
    NONFINITE = 5


# Margin: twice the largest ratio of the plain fp64 restatement's own error (fit_np against the 50-digit minimiser) to the
# scale below, over every scene, never below 4 -- the protocol of M_TETHER in tether_reference.py.
# Measured (test_fit_reference_host.py prints them): largest ratio 0.4225 for an angle (a 1 mm noise frame; 0.0033 on the
# noise-free frames), 0.0019 for the rms; twice that is below 4.
M_FIT = 4.0


def _mp(x):
    return mpf(float(x))


# ---- the model at 50 digits, with angles of any precision ---------------------------------------------------------------

def points_mp(A, P, th, ga, L, M, up, c_lo, c_hi):
    """tether_reference.node_points for mpf angles (that one rounds its angles to double: they are a kernel's stored
    values there, an unknown here).  Returns (points relative to A, kappa', root C' or None, chord)."""
    rel = [P[i] - A[i] for i in range(3)]
    th_axis, ga_axis = cr._axes(rel)
    Bp = cr._rod(rel, th_axis, th)
    lp = mp.sqrt(Bp[0] ** 2 + Bp[1] ** 2)
    dHp = up * Bp[2]
    root = cr._root_mp(lp, dHp, L)
    if root is None or not (c_lo <= root[1] <= c_hi):
        return [[mpf(m) / (M - 1) * r for r in rel] for m in range(M)], 0.0, None if root is None else root[1], True
    u, C, r = root
    x0 = lp / 2 - mp.atanh(dHp / L) / C
    ch0 = mp.cosh(C * x0)
    R = tr._matmul(tr._rot_matrix(ga_axis, mp.cos(ga), mp.sin(ga)), tr._rot_matrix(th_axis, mp.cos(th), -mp.sin(th)))
    pts = []
    for m in range(M):
        t = mpf(m) / (M - 1)
        pts.append(tr._apply(R, [t * Bp[0], t * Bp[1], up * (mp.cosh(C * (lp * t - x0)) - ch0) / C]))
    return pts, float(cr._kappa_mp(u, r, dHp, L)), C, False


MpFit = collections.namedtuple("MpFit", "theta gamma rms J kappa rootC steps")


def _jac_mp(A, P, th, ga, L, M, up, c_lo, c_hi):
    """(points, d/dtheta, d/dgamma) at 50 digits: both columns by central differences with h = 1e-15 (truncation 1e-30)."""
    h = mpf(10) ** -15
    pts, kap, C, chord = points_mp(A, P, th, ga, L, M, up, c_lo, c_hi)
    cols = []
    for dt, dg in ((h, 0), (0, h)):
        hi = points_mp(A, P, th + dt, ga + dg, L, M, up, c_lo, c_hi)[0]
        lo = points_mp(A, P, th - dt, ga - dg, L, M, up, c_lo, c_hi)[0]
        cols.append([[(hi[m][i] - lo[m][i]) / (2 * h) for i in range(3)] for m in range(M)])
    return pts, cols[0], cols[1], kap, C, chord


def fit_mp(A, P, Y, start, L=L_WS, up=1.0, bracket=BRACKET):
    """The 50-digit minimiser of F from `start` (the truth, or near it): Gauss-Newton on the 50-digit Jacobian until the step
    is below 1e-24 rad.  A, P (3,), Y (M, 3) doubles, NaN rows missing.  Returns MpFit: the angles and rms as mpf, the
    weighted Jacobian there as a float array (3 M, 2), the solve's kappa' and root there, and the steps taken."""
    Y = np.asarray(Y, dtype=np.float64)
    M = len(Y)
    w = np.isfinite(Y).all(axis=1)
    with mp.workdps(DPS):
        Am, Pm = [_mp(x) for x in A], [_mp(x) for x in P]
        Lm, upm, c_lo, c_hi = _mp(L), _mp(up), _mp(bracket[0]), _mp(bracket[1])
        y = [[_mp(Y[m, i]) - Am[i] if w[m] else mpf(0) for i in range(3)] for m in range(M)]
        th, ga = mpf(start[0]), mpf(start[1])
        for step in range(400):
            pts, jt, jg, kap, C, chord = _jac_mp(Am, Pm, th, ga, Lm, M, upm, c_lo, c_hi)
            if chord:
                raise RuntimeError("the 50-digit fit met the chord")
            a = b = c = g0 = g1 = F = mpf(0)
            for m in range(M):
                if not w[m]:
                    continue
                r = [pts[m][i] - y[m][i] for i in range(3)]
                for i in range(3):
                    a += jt[m][i] ** 2; b += jt[m][i] * jg[m][i]; c += jg[m][i] ** 2
                    g0 += jt[m][i] * r[i]; g1 += jg[m][i] * r[i]; F += r[i] ** 2
            d = a * c - b * b
            dth, dga = (g1 * b - g0 * c) / d, (g0 * b - g1 * a) / d
            if max(abs(dth), abs(dga)) < mpf(10) ** -24:
                break
            th, ga = th + dth, ga + dga
        else:
            raise RuntimeError("the 50-digit fit did not converge")
        J = np.array([[float(jt[m][i]), float(jg[m][i])] for m in range(M) if w[m] for i in range(3)])
        return MpFit(th, ga, mp.sqrt(F / int(w.sum())), J, kap, None if C is None else float(C), step)


# ---- the plain fp64 restatement -----------------------------------------------------------------------------------------

def model_np(rel, th, ga, L, M, up, bracket):
    """The model of the law in plain fp64 NumPy in the oracle's style (tether_reference.tether_np's node): X - A (M, 3) and the
    flag 1.0 (catenary), 0.0 (chord) or NaN (non-finite), and l' of the rotated end point."""
    from oracle import rovmpc_oracle as orc
    rel = np.asarray(rel, dtype=np.float64)[None]
    th, ga = np.array([th], dtype=np.float64), np.array([ga], dtype=np.float64)
    with np.errstate(all="ignore"):
        th_axis, ga_axis = orc._axes_vec(rel)
        Bp = orc._rod_vec(rel, th_axis, th)
        lp = np.sqrt(Bp[:, 0] ** 2 + Bp[:, 1] ** 2)
        dHp = up * Bp[:, 2]
        Cp = orc.solve_catenary_vec(lp, dHp, L, bracket[0], bracket[1])
        valid = bool(np.isfinite(Cp)[0])
        Cq = np.where(valid, Cp, 1.0)
        uq = 0.5 * lp * Cq
        ath = np.arctanh(np.where(valid, dHp / L, 0.0))
        X = np.empty((M, 3))
        for m in range(M):
            t = m / (M - 1)
            q = np.stack([t * Bp[:, 0], t * Bp[:, 1], up * (2.0 * np.sinh(uq * t) * np.sinh(uq * (t - 1.0) + ath)) / Cq], axis=1)
            q = orc._rod_vec(orc._rod_vec(q, th_axis, -th), ga_axis, ga)
            X[m] = q[0] if valid else t * rel[0]
    if not (np.isfinite(th[0]) and np.isfinite(ga[0]) and np.isfinite(ga_axis).all()):
        return np.full((M, 3), np.nan), np.nan, float(lp[0])
    return X, (1.0 if valid else 0.0), float(lp[0])


def _butterfly(s):
    """The 16-lane xor butterfly of the law (8, 4, 2, 1) on the M values of s, the other slots 0."""
    v = np.zeros(16)
    v[:len(s)] = s
    idx = np.arange(16)
    for k in (8, 4, 2, 1):
        v = v + v[idx ^ k]
    return v[0]


def _sums_np(rel, th, ga, y, w, L, M, up, bracket):
    """(usable, a, b, c, g0, g1, F, vertical) of the law at (th, ga)."""
    X0, f0, lp0 = model_np(rel, th, ga, L, M, up, bracket)
    Xp, fp, _ = model_np(rel, th + H, ga, L, M, up, bracket)
    Xm, fm, _ = model_np(rel, th - H, ga, L, M, up, bracket)
    usable = f0 == 1.0 and fp == 1.0 and fm == 1.0
    with np.errstate(all="ignore"):
        jt = (Xp - Xm) * (0.5 / H)
        jg = np.cross(rel / np.linalg.norm(rel), X0)
        r = X0 - y
        dot = lambda p, q: np.where(w, p[:, 0] * q[:, 0] + (p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2]), 0.0)
        return (usable,) + tuple(_butterfly(dot(p, q)) for p, q in ((jt, jt), (jt, jg), (jg, jg), (jt, r), (jg, r), (r, r))) + (lp0 == 0.0,)


def fit_np(A, P, Y, guess=None, L=L_WS, up=1.0, bracket=BRACKET, tol=TOL, max_iter=MAX_ITER):
    """The header's iteration for one frame in plain fp64: [theta, gamma, rms, rms0, trial steps, status]."""
    A, P, Y = np.asarray(A, dtype=np.float64), np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    M = len(Y)
    th, ga = (0.0, 0.0) if guess is None else (float(guess[0]), float(guess[1]))
    with np.errstate(all="ignore"):
        rel = P - A
        y = Y - A
    w = np.isfinite(y).all(axis=1)
    if not (np.isfinite(A).all() and np.isfinite(rel).all() and math.isfinite(th) and math.isfinite(ga)) or not rel.any():
        return np.array([np.nan, np.nan, np.nan, np.nan, 0.0, Status.NONFINITE])
    nw = float(w.sum())
    args = (y, w, L, M, up, bracket)
    usable, a, b, c, g0, g1, F, vertical = _sums_np(rel, th, ga, *args)
    F0, iters, mu, status = F, 0, MU0, None
    with np.errstate(all="ignore"):
        if not w[1:-1].any():
            status = Status.TOO_FEW
        elif not usable:
            status = Status.DEGENERATE if vertical else Status.CHORD
        elif not (a * c - b * b > DET_MIN * a * c):
            status = Status.DEGENERATE
        while status is None:
            if iters >= max_iter:
                status = Status.MAX_ITER
                break
            ad, cd = a * (1.0 + mu), c * (1.0 + mu)
            d = 1.0 / (ad * cd - b * b)
            dth, dga = (g1 * b - g0 * cd) * d, (g0 * b - g1 * ad) * d
            tht, gat = th + dth, ga + dga
            ok, at, bt, ct, g0t, g1t, Ft, _ = _sums_np(rel, tht, gat, *args)
            iters += 1
            moved = bool(ok and Ft <= F + SLACK * L * math.sqrt(nw * F))
            if moved:
                th, ga, a, b, c, g0, g1, F = tht, gat, at, bt, ct, g0t, g1t, Ft
                mu = max(mu * 0.1, MU_MIN)
            else:
                mu = mu * 10.0
            if max(abs(dth), abs(dga)) <= tol:
                status = Status.CONVERGED
            elif moved and not (a * c - b * b > DET_MIN * a * c):
                status = Status.DEGENERATE
        return np.array([th, ga, math.sqrt(F / nw) if nw else np.nan, math.sqrt(F0 / nw) if nw else np.nan, float(iters), float(status)])


# ---- the scenes ---------------------------------------------------------------------------------------------------------

Frame = collections.namedtuple("Frame", "name geom A P Y guess M up max_iter truth noisy")

ANCHOR = tr.ANCHOR
WELL_POSED = tuple(i for i in range(20) if i not in (13, 18))
OFFSETS = ((0.15, -0.2), (-0.2, 0.15))


def truth_of(i):
    return 0.3 * math.sin(1.3 * i + 0.2), 0.5 * math.cos(0.9 * i)


def make_frame(name, i, M=16, up=1.0, A=(0.0, 0.0, 0.0), guess=(0.0, 0.0), missing=(), noise=0.0, max_iter=MAX_ITER, seed=0):
    """Geometry i of cable_reference.shape_geometry() (mirrored in z for NED) at its truth: markers at 50 digits rounded to
    fp64, plus seeded Gaussian noise of `noise` metres on the interior markers, rows `missing` NaN."""
    g = cr.shape_geometry(L_WS)[i]
    A = np.asarray(A, dtype=np.float64)
    P = A + np.array([g[0], g[1], up * g[2]])
    th, ga = truth_of(i)
    with mp.workdps(DPS):
        Am, Pm = [_mp(x) for x in A], [_mp(x) for x in P]
        pts = tr.node_points(Am, Pm, th, ga, _mp(L_WS), M, _mp(up), _mp(BRACKET[0]), _mp(BRACKET[1]))[0]
        Y = np.array([[float(Am[j] + p[j]) for j in range(3)] for p in pts])
    if noise:
        Y[1:-1] += noise * np.random.default_rng(seed).standard_normal((M - 2, 3))
    Y[list(missing)] = np.nan
    return Frame(name, i, A, P, Y, None if guess is None else np.asarray(guess, dtype=np.float64), M, up, max_iter, (th, ga), bool(noise))


@functools.lru_cache(maxsize=None)
def scenes():
    """The frames (fewer than 80), in a fixed order."""
    fr = [make_frame(f"g{i}", i) for i in WELL_POSED]
    for i in (18, 20):                                                       # steep and vertical: local fits from near the truth
        t = truth_of(i)
        fr += [make_frame(f"g{i}-start{k}", i, guess=(t[0] + o[0], t[1] + o[1])) for k, o in enumerate(OFFSETS)]
    fr += [make_frame(f"g{i}-M{M}", i, M=M) for M in (3, 5) for i in (6, 9, 11)]
    fr += [make_frame(f"g{i}-ned", i, up=-1.0) for i in (4, 7, 10, 14)]
    fr += [make_frame(f"g{i}-anchor", i, A=ANCHOR) for i in (2, 5, 8, 19)]
    fr += [make_frame("g7-miss1", 7, missing=(7,)), make_frame("g10-miss5", 10, missing=(0, 3, 8, 9, 15)),
           make_frame("g4-miss13", 4, missing=tuple(m for m in range(16) if m not in (4, 9, 12)))]
    # one frame per status that does not iterate, and one cut off after a single trial step
    nan_P = make_frame("nonfinite-P", 6)
    fr.append(nan_P._replace(P=np.array([nan_P.P[0], np.nan, nan_P.P[2]]), truth=None))
    zero = make_frame("nonfinite-rel0", 6, A=ANCHOR)
    fr.append(zero._replace(P=zero.A.copy(), truth=None))
    fr.append(make_frame("too-few", 6, guess=(0.1, -0.2), missing=tuple(range(1, 15)))._replace(truth=None))
    fr.append(make_frame("chord", 21, guess=None)._replace(truth=None))
    fr.append(make_frame("degenerate", 20)._replace(truth=None))
    fr.append(make_frame("max-iter", 6, max_iter=1)._replace(truth=None))
    fr += [make_frame(f"g{i}-noise", i, noise=1e-3, seed=100 + i) for i in range(4, 12)]
    assert len(fr) <= 80 and len({f.name for f in fr}) == len(fr)
    return tuple(fr)


Ref = collections.namedtuple("Ref", "np_out status mp sigma jnorm scale")


def scale_of(frame, kappa, sigma, tol=TOL):
    """s = 2^-52 (1 + kappa') (L + |A| + max |Y|) / sigma + tol."""
    ymax = np.nanmax(np.linalg.norm(frame.Y, axis=1))
    return EPS * (1.0 + kappa) * (L_WS + np.linalg.norm(frame.A) + ymax) / sigma + tol


@functools.lru_cache(maxsize=None)
def references():
    """Per frame: fit_np's row and status; where that is CONVERGED and the frame has a truth, the 50-digit minimiser from the
    truth, the singular values (sigma the smaller, jnorm the larger) of its weighted Jacobian and the error scale s."""
    out = []
    for f in scenes():
        row = fit_np(f.A, f.P, f.Y, f.guess, up=f.up, max_iter=f.max_iter)
        status = Status(int(row[5]))
        m = sigma = jnorm = s = None
        if status is Status.CONVERGED and f.truth is not None:
            m = fit_mp(f.A, f.P, f.Y, f.truth, up=f.up)
            sv = np.linalg.svd(m.J, compute_uv=False)
            sigma, jnorm = float(sv[-1]), float(sv[0])
            s = scale_of(f, m.kappa, sigma)
        out.append(Ref(row, status, m, sigma, jnorm, s))
    return tuple(out)


def angle_errors(theta, gamma, ref):
    """(|theta - theta_ref|, |gamma - gamma_ref|) against the 50-digit minimiser, as floats."""
    with mp.workdps(DPS):
        return float(abs(_mp(theta) - ref.mp.theta)), float(abs(_mp(gamma) - ref.mp.gamma))


def rms_error(rms, ref):
    """(|rms - rms_ref|, its allowance beyond m s |J|: one ulp of the reference's rms)."""
    with mp.workdps(DPS):
        return float(abs(_mp(rms) - ref.mp.rms)), float(np.spacing(float(ref.mp.rms)))


@functools.lru_cache(maxsize=None)
def start_rms(k):
    """rms0 of scene k at 50 digits and the allowance of an fp64 evaluation: M_TETHER 2^-52 (1 + kappa') (L + |A| + max |Y|)
    with the start's kappa' -- the rms is 1-Lipschitz in the points, which tests/test_tether_gpu.py holds to that margin.
    (None, None) for a frame without a valid marker or with a non-finite input."""
    f = scenes()[k]
    w = np.isfinite(f.Y).all(axis=1)
    if not (w.any() and np.isfinite(f.P).all() and (f.P - f.A).any()):
        return None, None
    th, ga = (0.0, 0.0) if f.guess is None else f.guess
    with mp.workdps(DPS):
        Am, Pm = [_mp(x) for x in f.A], [_mp(x) for x in f.P]
        pts, kap, _, _ = points_mp(Am, Pm, _mp(th), _mp(ga), _mp(L_WS), f.M, _mp(f.up), _mp(BRACKET[0]), _mp(BRACKET[1]))
        F = sum((pts[m][i] - (_mp(f.Y[m, i]) - Am[i])) ** 2 for m in range(f.M) if w[m] for i in range(3))
        rms = mp.sqrt(F / int(w.sum()))
    size = L_WS + np.linalg.norm(f.A) + np.nanmax(np.linalg.norm(f.Y, axis=1))
    return rms, tr.M_TETHER * EPS * (1.0 + kap) * size + float(np.spacing(float(rms)))
