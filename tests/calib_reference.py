"""Reference of the cable-length calibration (law: include/rovmpc.h above rovmpc_calibrate_cable): the forward model with the
markers placed by arc length at 50 digits (`markers_mp`) and in plain fp64 NumPy (`markers_np`), the law's iteration
operation by operation in NumPy (`calib_np`, one group), the 50-digit joint minimiser (`calib_mp`), and the cases both the
host test and the GPU test run.  Imports fit_reference, cable_reference and tether_reference as they stand."""
import collections
import functools
import json
import math
import os

import numpy as np
from mpmath import mp, mpf

import cable_reference as cr
import fit_reference as fr
import tether_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DPS, EPS, L_WS, BRACKET = fr.DPS, fr.EPS, fr.L_WS, fr.BRACKET
H, MU0, MU_MIN, DET_MIN, SLACK = fr.H, fr.MU0, fr.MU_MIN, fr.DET_MIN, fr.SLACK
MU_MAX = 1e12
TILE = 128
TOL, TOL_L, MAX_ITER = 1e-12, 1e-12, 60
CONVERGED, MAX_ITER_S, DEGENERATE, CHORD, TOO_FEW, NONFINITE, STALLED, NO_FRAMES = range(8)
_mp = fr._mp


def bounds():
    with open(os.path.join(GOLDEN, "calib_bounds.json")) as f:
        return json.load(f)


def uniform_arc(M):
    return np.arange(M) / (M - 1.0)


def uneven_arc(M):
    """Strictly increasing from 0 to 1, denser towards the far end."""
    s = (np.arange(M) / (M - 1.0)) ** 0.6
    s[0], s[-1] = 0.0, 1.0
    return s


# ---- the forward model ----------------------------------------------------------------------------------------------------

def asinh_np(x):
    """The law's asinh: sign(x) log1p(|x| + x^2 / (1 + sqrt(1 + x^2)))."""
    a = np.abs(x)
    return np.sign(x) * np.log1p(a + a * a / (1.0 + np.sqrt(1.0 + a * a)))


def model_vec(rel, th, ga, L, M, up=1.0, bracket=BRACKET, arc=None, root_C=None):
    """The law's model for F frames at once in plain fp64 NumPy, in the style of fit_reference.model_np: X - A (F, M, 3), the
    flag (F,) 1.0 catenary / 0.0 chord / NaN non-finite, and l' (F,).  rel (F, 3); th, ga (F,); L a scalar or (F,).  `root_C`:
    the root C' given instead of solved for (cables beyond the oracle solver's reach)."""
    from oracle import rovmpc_oracle as orc
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3)
    F = len(rel)
    th, ga = np.broadcast_to(np.asarray(th, np.float64), (F,)).copy(), np.broadcast_to(np.asarray(ga, np.float64), (F,)).copy()
    L = np.broadcast_to(np.asarray(L, np.float64), (F,)).copy()
    with np.errstate(all="ignore"):
        th_axis, ga_axis = orc._axes_vec(rel)
        Bp = orc._rod_vec(rel, th_axis, th)
        lp = np.sqrt(Bp[:, 0] ** 2 + Bp[:, 1] ** 2)
        dHp = up * Bp[:, 2]
        Cp = orc.solve_catenary_vec(lp, dHp, L, bracket[0], bracket[1]) if root_C is None else np.broadcast_to(np.asarray(root_C, np.float64), (F,))
        valid = np.isfinite(Cp)
        Cq = np.where(valid, Cp, 1.0)
        uq = 0.5 * lp * Cq
        ath = np.arctanh(np.where(valid, dHp / L, 0.0))
        X = np.empty((F, M, 3))
        for m in range(M):
            if arc is None:
                t = np.full(F, m / (M - 1))
                tc = t
            else:
                tc = np.full(F, float(arc[m]))
                w = uq - ath
                t = (w + asinh_np(arc[m] * ((2.0 * L) / (2.0 / Cq)) - np.sinh(w))) / (2.0 * uq)
                if m == 0:
                    t = np.zeros(F)
                elif m == M - 1:
                    t = np.ones(F)
            q = np.stack([t * Bp[:, 0], t * Bp[:, 1], up * (2.0 * np.sinh(uq * t) * np.sinh(uq * (t - 1.0) + ath)) / Cq], axis=1)
            q = orc._rod_vec(orc._rod_vec(q, th_axis, -th), ga_axis, ga)
            X[:, m] = np.where(valid[:, None], q, tc[:, None] * rel)
        bad = ~(np.isfinite(th) & np.isfinite(ga) & np.isfinite(ga_axis).all(axis=1))
        X[bad] = np.nan
        flag = np.where(bad, np.nan, np.where(valid, 1.0, 0.0))
    return X, flag, lp


def markers_np(P0, P1, theta, gamma, L=L_WS, arc=None, M=16, up=1.0, bracket=BRACKET, root_C=None):
    """rovmpc_cable_markers in plain fp64 NumPy: (B, M, 3)."""
    P0, P1 = np.asarray(P0, np.float64).reshape(-1, 3), np.asarray(P1, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        X, _, _ = model_vec(P1 - P0, theta, gamma, L, M, up, bracket, arc, root_C)
        return X + P0[:, None, :]


def points_mp(A, P, th, ga, L, M, up, c_lo, c_hi, arc=None):
    """fit_reference.points_mp with the law's placement: the points relative to A (mpf), and whether it is the chord.  With
    `arc` marker m sits where the cable's arc from A is arc[m] L, by the closed inversion, evaluated at 50 digits."""
    rel = [P[i] - A[i] for i in range(3)]
    th_axis, ga_axis = cr._axes(rel)
    Bp = cr._rod(rel, th_axis, th)
    lp = mp.sqrt(Bp[0] ** 2 + Bp[1] ** 2)
    dHp = up * Bp[2]
    root = cr._root_mp(lp, dHp, L)
    s = [mpf(m) / (M - 1) for m in range(M)] if arc is None else [_mp(x) for x in arc]
    if root is None or not (c_lo <= root[1] <= c_hi):
        return [[s[m] * r for r in rel] for m in range(M)], True
    u, C, r = root
    ath = mp.atanh(dHp / L)
    x0 = lp / 2 - ath / C
    ch0 = mp.cosh(C * x0)
    R = tr._matmul(tr._rot_matrix(ga_axis, mp.cos(ga), mp.sin(ga)), tr._rot_matrix(th_axis, mp.cos(th), -mp.sin(th)))
    pts = []
    for m in range(M):
        if arc is None or m == 0 or m == M - 1:
            t = mpf(m) / (M - 1)
        else:
            w = u - ath
            t = (w + mp.asinh(s[m] * C * L - mp.sinh(w))) / (2 * u)
        pts.append(tr._apply(R, [t * Bp[0], t * Bp[1], up * (mp.cosh(C * (lp * t - x0)) - ch0) / C]))
    return pts, False


def markers_mp(P0, P1, theta, gamma, L=L_WS, arc=None, M=16, up=1.0, bracket=BRACKET):
    """One cable at 50 digits (inputs are doubles): the points (M, 3) as mpf, absolute, and whether it is the chord."""
    with mp.workdps(DPS):
        A, P = [_mp(x) for x in P0], [_mp(x) for x in P1]
        pts, chord = points_mp(A, P, _mp(theta), _mp(gamma), _mp(L), M, _mp(up), _mp(bracket[0]), _mp(bracket[1]), arc)
        return [[A[i] + p[i] for i in range(3)] for p in pts], chord


def arc_integral_mp(P0, P1, theta, gamma, L, t, up=1.0):
    """The cable's arc from A to the chord parameter t by numerical quadrature of the catenary's line element at 50 digits:
    an independent check of the placement's inversion."""
    with mp.workdps(DPS):
        A, P = [_mp(x) for x in P0], [_mp(x) for x in P1]
        rel = [P[i] - A[i] for i in range(3)]
        th_axis, _ = cr._axes(rel)
        Bp = cr._rod(rel, th_axis, _mp(theta))
        lp = mp.sqrt(Bp[0] ** 2 + Bp[1] ** 2)
        dHp = _mp(up) * Bp[2]
        u, C, r = cr._root_mp(lp, dHp, _mp(L))
        x0 = lp / 2 - mp.atanh(dHp / _mp(L)) / C
        return mp.quad(lambda x: mp.sqrt(1 + mp.sinh(C * (x - x0)) ** 2), [0, lp * t])


def chord_parameter_mp(P0, P1, theta, gamma, L, s, up=1.0):
    """t of the law's placement at 50 digits for the arc fraction s."""
    with mp.workdps(DPS):
        A, P = [_mp(x) for x in P0], [_mp(x) for x in P1]
        rel = [P[i] - A[i] for i in range(3)]
        th_axis, _ = cr._axes(rel)
        Bp = cr._rod(rel, th_axis, _mp(theta))
        lp = mp.sqrt(Bp[0] ** 2 + Bp[1] ** 2)
        dHp = _mp(up) * Bp[2]
        u, C, r = cr._root_mp(lp, dHp, _mp(L))
        w = u - mp.atanh(dHp / _mp(L))
        return (w + mp.asinh(_mp(s) * C * _mp(L) - mp.sinh(w))) / (2 * u)


# ---- the law's iteration in NumPy -------------------------------------------------------------------------------------------

def _butterfly_vec(s):
    """fit_reference._butterfly for F frames: s (F, M) -> (F,)."""
    v = np.zeros((len(s), 16))
    v[:, :s.shape[1]] = s
    idx = np.arange(16)
    for k in (8, 4, 2, 1):
        v = v + v[:, idx ^ k]
    return v[:, 0]


def tree_sum(x):
    """The law's sum over a group's frames: tiles of 128, the tree of rovmpc_score_rows inside, tile sums in order from +0."""
    x = np.asarray(x, dtype=np.float64)
    tot = 0.0
    for t0 in range(0, len(x), TILE):
        v = np.zeros(TILE)
        v[:len(x[t0:t0 + TILE])] = x[t0:t0 + TILE]
        s = TILE // 2
        while s >= 1:
            v[:s] = v[:s] + v[s:2 * s]
            s //= 2
        tot = tot + v[0]
    return tot


def frame_sums(rel, th, ga, L, y, w, M, up, bracket, arc, free_length):
    """(usable (F,), sums (F, 10): a b c g0 g1 F p0 p1 d gL, vertical (F,)) of the law at (th, ga, L)."""
    X0, f0, lp0 = model_vec(rel, th, ga, L, M, up, bracket, arc)
    Xp, fp, _ = model_vec(rel, th + H, ga, L, M, up, bracket, arc)
    Xm, fm, _ = model_vec(rel, th - H, ga, L, M, up, bracket, arc)
    usable = (f0 == 1.0) & (fp == 1.0) & (fm == 1.0)
    with np.errstate(all="ignore"):
        jt = (Xp - Xm) * (0.5 / H)
        k = rel / np.linalg.norm(rel, axis=1, keepdims=True)
        jg = np.cross(k[:, None, :], X0)
        r = X0 - y
        dot = lambda p, q: np.where(w, p[..., 0] * q[..., 0] + (p[..., 1] * q[..., 1] + p[..., 2] * q[..., 2]), 0.0)
        cols = [(jt, jt), (jt, jg), (jg, jg), (jt, r), (jg, r), (r, r)]
        if free_length:
            Xlp, flp, _ = model_vec(rel, th, ga, L + H, M, up, bracket, arc)
            Xlm, flm, _ = model_vec(rel, th, ga, L - H, M, up, bracket, arc)
            usable &= (flp == 1.0) & (flm == 1.0)
            jl = (Xlp - Xlm) * (0.5 / H)
            cols += [(jt, jl), (jg, jl), (jl, jl), (jl, r)]
        S = np.zeros((len(rel), 10))
        for i, (p, q) in enumerate(cols):
            S[:, i] = _butterfly_vec(dot(p, q))
    return usable, S, lp0 == 0.0


def _solve(a, b, c, g0, g1, mu):
    ad, cd = a * (1.0 + mu), c * (1.0 + mu)
    d = 1.0 / (ad * cd - b * b)
    return (g1 * b - g0 * cd) * d, (g0 * b - g1 * ad) * d


CalibOut = collections.namedtuple("CalibOut", "group frames")


def calib_np(P0, P1, Y, guess=None, arc=None, L0=L_WS, free_length=True, L_lo=0.0, L_hi=math.inf, tol=TOL, tol_L=TOL_L, max_iter=MAX_ITER,
             up=1.0, bracket=BRACKET):
    """The law for ONE group in plain fp64 NumPy: CalibOut(group row (8,), frame rows (F, 5))."""
    P0, P1, Y = (np.asarray(x, dtype=np.float64) for x in (P0, P1, Y))
    F, M = Y.shape[:2]
    out_f = np.full((F, 5), np.nan)
    th = np.zeros(F) if guess is None else np.asarray(guess, np.float64)[:, 0].copy()
    ga = np.zeros(F) if guess is None else np.asarray(guess, np.float64)[:, 1].copy()
    with np.errstate(all="ignore"):
        rel, y = P1 - P0, Y - P0[:, None, :]
        w = np.isfinite(y).all(axis=2)
        nw = w.sum(axis=1).astype(np.float64)
        cls = np.full(F, -1)
        nonfinite = ~(np.isfinite(P0).all(axis=1) & np.isfinite(rel).all(axis=1) & np.isfinite(th) & np.isfinite(ga)) | ~rel.any(axis=1)
        L = float(L0)
        usable, S, vertical = frame_sums(rel, th, ga, L, y, w, M, up, bracket, arc, free_length)
        det_bad = ~(S[:, 0] * S[:, 2] - S[:, 1] ** 2 > DET_MIN * S[:, 0] * S[:, 2])
        for f in range(F):
            if nonfinite[f]:
                cls[f] = NONFINITE
            elif not w[f, 1:-1].any():
                cls[f] = TOO_FEW
            elif not usable[f]:
                cls[f] = DEGENERATE if vertical[f] else CHORD
            elif det_bad[f]:
                cls[f] = DEGENERATE
            if cls[f] == NONFINITE:
                out_f[f] = [np.nan] * 4 + [NONFINITE]
            elif cls[f] != -1:
                rms = math.sqrt(S[f, 5] / nw[f]) if nw[f] else np.nan
                out_f[f] = [th[f], ga[f], rms, rms, cls[f]]
        act = cls == -1
        z = lambda x: np.where(act, x, 0.0)
        Nw, nact = tree_sum(z(nw)), float(act.sum())
        if nact == 0:
            return CalibOut(np.array([L, np.nan, np.nan, np.nan, 0.0, NO_FRAMES, 0.0, 0.0]), out_f)
        F0f = S[:, 5].copy()
        Fg = F0 = tree_sum(z(S[:, 5]))
        mu, iters, status, moved = MU0, 0, None, True
        dL = 0.0
        while True:
            y0, y1 = _solve(S[:, 0], S[:, 1], S[:, 2], S[:, 3], S[:, 4], mu)
            z0, z1 = _solve(S[:, 0], S[:, 1], S[:, 2], S[:, 6], S[:, 7], mu)
            w0, w1 = _solve(S[:, 0], S[:, 1], S[:, 2], S[:, 6], S[:, 7], 0.0)
            Sd = tree_sum(z(S[:, 8]))
            Ss = (1.0 + mu) * Sd + tree_sum(z(S[:, 6] * z0 + S[:, 7] * z1))
            R = tree_sum(z(S[:, 9])) + tree_sum(z(S[:, 6] * y0 + S[:, 7] * y1))
            S0 = Sd + tree_sum(z(S[:, 6] * w0 + S[:, 7] * w1))
            if status is None and moved:
                if free_length and not (Ss > DET_MIN * (1.0 + mu) * Sd):
                    status = DEGENERATE
                elif (act & ~(S[:, 0] * S[:, 2] - S[:, 1] ** 2 > DET_MIN * S[:, 0] * S[:, 2])).any():
                    status = DEGENERATE
            if status is None and iters >= max_iter:
                status = MAX_ITER_S
            if status is None and mu > MU_MAX:
                status = STALLED
            if status is not None:
                break
            dL = -R / Ss if free_length else 0.0
            dth, dga = (y0 + z0 * dL, y1 + z1 * dL) if free_length else (y0, y1)
            tht, gat, Lt = np.where(act, th + dth, th), np.where(act, ga + dga, ga), L + dL
            small = bool((np.maximum(np.abs(dth), np.abs(dga)) <= tol)[act].all())
            ok, St, _ = frame_sums(rel, tht, gat, Lt, y, w, M, up, bracket, arc, free_length)
            iters += 1
            Ft = tree_sum(z(St[:, 5]))
            moved = bool(ok[act].all() and L_lo < Lt < L_hi and Ft <= Fg + (SLACK * L) * math.sqrt(Nw * Fg))
            if moved:
                th, ga, L, S, Fg = tht, gat, Lt, np.where(act[:, None], St, S), Ft
                mu = max(mu * 0.1, MU_MIN)
            else:
                mu = mu * 10.0
            if small and abs(dL) <= tol_L:
                status = CONVERGED
        for f in np.nonzero(act)[0]:
            out_f[f] = [th[f], ga[f], math.sqrt(S[f, 5] / nw[f]), math.sqrt(F0f[f] / nw[f]), status]
        dof = 3.0 * Nw - 2.0 * nact - 1.0
        sigma = math.sqrt(Fg / dof / S0) if free_length and dof > 0 else np.nan
        return CalibOut(np.array([L, math.sqrt(Fg / Nw), math.sqrt(F0 / Nw), sigma, float(iters), float(status), nact, Nw]), out_f)


# ---- the 50-digit joint minimiser --------------------------------------------------------------------------------------------

MpCalib = collections.namedtuple("MpCalib", "L theta gamma grad steps")


def _frame_mp(A, P, y, w, th, ga, L, M, up, c_lo, c_hi, arc, h):
    """Residuals and the three Jacobian columns (theta, gamma, L) of one frame at 50 digits by central differences."""
    def pts(t, g, l):
        p, chord = points_mp(A, P, t, g, l, M, up, c_lo, c_hi, arc)
        if chord:
            raise RuntimeError("the 50-digit model met the chord")
        return p
    p0 = pts(th, ga, L)
    cols = []
    for dt, dg, dl in ((h, 0, 0), (0, h, 0), (0, 0, h)):
        hi, lo = pts(th + dt, ga + dg, L + dl), pts(th - dt, ga - dg, L - dl)
        cols.append([[(hi[m][i] - lo[m][i]) / (2 * h) for i in range(3)] for m in range(M)])
    r = [[p0[m][i] - y[m][i] for i in range(3)] for m in range(M)]
    idx = [(m, i) for m in range(M) if w[m] for i in range(3)]
    dot = lambda p, q: sum((p[m][i] * q[m][i] for m, i in idx), mpf(0))
    jt, jg, jl = cols
    return dict(a=dot(jt, jt), b=dot(jt, jg), c=dot(jg, jg), g0=dot(jt, r), g1=dot(jg, r), p0=dot(jt, jl), p1=dot(jg, jl), d=dot(jl, jl),
                gL=dot(jl, r), F=dot(r, r))


def calib_mp(P0, P1, Y, theta, gamma, L, arc=None, up=1.0, bracket=BRACKET, max_steps=40, stop=mpf(10) ** -22, steps=True):
    """The 50-digit minimiser of the pooled F over (L, theta_t, gamma_t) from the given start: Gauss-Newton by the Schur
    complement until every step is below `stop`; with steps=False only the gradient at the start is formed.  Returns MpCalib
    with L, theta, gamma as mpf and `grad` = the largest |component| of J^T r there (metres^2 per unit), as a float."""
    Y = np.asarray(Y, dtype=np.float64)
    F, M = Y.shape[:2]
    w = np.isfinite(Y).all(axis=2)
    with mp.workdps(DPS):
        h = mpf(10) ** -15
        upm, c_lo, c_hi = _mp(up), _mp(bracket[0]), _mp(bracket[1])
        A = [[_mp(x) for x in P0[f]] for f in range(F)]
        P = [[_mp(x) for x in P1[f]] for f in range(F)]
        y = [[[_mp(Y[f, m, i]) - A[f][i] if w[f, m] else mpf(0) for i in range(3)] for m in range(M)] for f in range(F)]
        th, ga, Lm = [mpf(t) for t in theta], [mpf(g) for g in gamma], mpf(L)
        for step in range(max_steps):
            fs = [_frame_mp(A[f], P[f], y[f], w[f], th[f], ga[f], Lm, M, upm, c_lo, c_hi, arc, h) for f in range(F)]
            grad = max([abs(sum(s["gL"] for s in fs))] + [max(abs(s["g0"]), abs(s["g1"])) for s in fs])
            if not steps:
                return MpCalib(Lm, th, ga, float(grad), 0)
            S = R = mpf(0)
            ys, zs = [], []
            for s in fs:
                det = s["a"] * s["c"] - s["b"] ** 2
                yv = ((s["g1"] * s["b"] - s["g0"] * s["c"]) / det, (s["g0"] * s["b"] - s["g1"] * s["a"]) / det)
                zv = ((s["p1"] * s["b"] - s["p0"] * s["c"]) / det, (s["p0"] * s["b"] - s["p1"] * s["a"]) / det)
                S += s["d"] + s["p0"] * zv[0] + s["p1"] * zv[1]
                R += s["gL"] + s["p0"] * yv[0] + s["p1"] * yv[1]
                ys.append(yv); zs.append(zv)
            dL = -R / S
            big = abs(dL)
            for f in range(F):
                dt, dg = ys[f][0] + zs[f][0] * dL, ys[f][1] + zs[f][1] * dL
                th[f] += dt; ga[f] += dg
                big = max(big, abs(dt), abs(dg))
            Lm += dL
            if big < stop:
                return MpCalib(Lm, th, ga, float(grad), step + 1)
        raise RuntimeError("the 50-digit calibration did not converge")


# ---- the cases ---------------------------------------------------------------------------------------------------------------

FORWARD_M = (3, 5, 16)


@functools.lru_cache(maxsize=None)
def forward_cases():
    """(name, P0, P1, theta, gamma, L): a symmetric chord, two steep ones (dH'/L near +-0.9), a nearly taut one, a slack one
    with the root close to c_hi, a chord case (longer than L) and a NaN angle."""
    c_hi = BRACKET[1]
    A = tr.ANCHOR
    cases = [("symmetric", (0, 0, 0), (1.6, 0.4, 0.0), 0.2, -0.3, 3.0),
             ("steep-up", (0, 0, 0), (0.5, 0.3, 2.68), 0.02, 0.3, 3.0),
             ("steep-down", A, A + np.array([0.4, -0.5, -2.66]), -0.02, 0.1, 3.0),
             ("taut", (0, 0, 0), (2.2, 1.6, 1.2), 0.0, 0.2, 3.0),
             ("slack", A, A + np.array([0.055, 0.04, 0.01]), 0.1, -0.2, 3.0),
             ("other-length", (0, 0, 0), (1.1, -0.7, 0.4), -0.25, 0.35, 2.7),
             ("chord", (0, 0, 0), (2.5, 1.5, 1.2), 0.1, 0.1, 3.0),
             ("nan-angle", (0, 0, 0), (1.0, 0.5, 0.2), float("nan"), 0.1, 3.0)]
    return tuple((n, np.asarray(a, float), np.asarray(p, float), t, g, l) for n, a, p, t, g, l in cases)


# The law's asinh, held through the forward model: level cables of 3 m (dH' = 0, so w = u and the argument of asinh is
# x = (2 s - 1) sinh(u) up to rounding) from nearly taut (u = 1e-4) to so slack that sinh(u) = e^16.75 / 2 > e^16, with arc
# fractions that take x from -sinh(u) through +-2^-47 sinh(u) (below 2^-60 on the taut cable) to +sinh(u): |x| from 2^-60
# to e^16.  The slack end needs C' = 2 u / l' up to 6.3e6, so every cable comes with a bracket of its own, c_hi =
# max(200, 4 u / l') (a bracket whose sinh(c_hi l' / 2) overflows is outside the oracle's solver).
ASINH_ARC = np.array([0.0, 2.0 ** -30, 0.1, 0.5 * (1 - 2.0 ** -20), 0.5 * (1 - 2.0 ** -47), 0.5, 0.5 * (1 + 2.0 ** -47),
                      0.5 * (1 + 2.0 ** -20), 0.9, 1 - 2.0 ** -30, 1.0])
ASINH_U = (1e-4, 0.5, 3.0, 8.0, 12.0, 14.0, 16.0, 16.75)
# Beyond u = 14 the oracle's NumPy solver loses the root; there the restatement is given the root (the 50-digit one, rounded:
# asinh_root), so that its error is measured over the whole range.
ASINH_U_NP = 14.0


def asinh_cases():
    """(P0, P1, theta, gamma, L, bracket, u) of the level cables: l' = L u / sinh(u)."""
    out = []
    for u in ASINH_U:
        lp = 3.0 * (1 - u * u / 6) if u < 1e-2 else 3.0 * u / math.sinh(u)
        out.append((np.zeros(3), np.array([lp, 0.0, 0.0]), 0.0, 0.0, 3.0, (1e-6, max(200.0, 4 * u / lp)), u))
    return tuple(out)


def asinh_root(case):
    """C' of a case the NumPy solver cannot do (None where it can): the 50-digit root rounded to fp64."""
    A, P, th, ga, L, _, u = case
    if u <= ASINH_U_NP:
        return None
    with mp.workdps(DPS):
        return float(cr._root_mp(_mp(P[0]), mpf(0), _mp(L))[1])


def asinh_arguments(case):
    """|x| of the placement's asinh for the interior markers of ASINH_ARC on `case` at 50 digits (floats), and the solve's
    kappa' there (the conditioning every point of the cable inherits from the root, as in fit_reference.scale_of)."""
    A, P, th, ga, L = case[:5]
    with mp.workdps(DPS):
        u, C, r = cr._root_mp(_mp(P[0]), mpf(0), _mp(L))
        return [float(abs(_mp(s) * C * _mp(L) - mp.sinh(u))) for s in ASINH_ARC[1:-1]], float(cr._kappa_mp(u, r, mpf(0), _mp(L)))


def recording(n, L_true, seed, M=16, noise=0.0, missing=0, arc="uniform", forward=markers_np):
    """n frames: chord radius 0.8..1.8 m, z +-0.6 m, theta +-0.3, gamma +-0.4, markers placed by
    arc length on a cable of L_true by `forward` (the NumPy forward model, or the engine's cable_markers with the same
    signature), starts 0.1 rad off, seeded."""
    rng = np.random.default_rng(seed)
    rad, az = rng.uniform(0.8, 1.8, n), rng.uniform(0, 2 * np.pi, n)
    P1 = np.stack([rad * np.cos(az), rad * np.sin(az), rng.uniform(-0.6, 0.6, n)], axis=1)
    P0 = np.zeros((n, 3))
    th, ga = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.4, 0.4, n)
    s = uniform_arc(M) if isinstance(arc, str) else arc
    Y = np.array(forward(P0, P1, th, ga, L_true, s, M))
    guess = np.stack([th, ga], axis=1) + 0.1 * rng.choice([-1.0, 1.0], (n, 2))
    if noise:
        Y[:, 1:-1] += noise * rng.standard_normal((n, M - 2, 3))
    for k in range(missing):
        f = int(rng.integers(0, n))
        Y[f, rng.choice(np.arange(1, M - 1), 3, replace=False)] = np.nan
    return dict(P0=P0, P1=P1, Y=Y, guess=guess, theta=th, gamma=ga, arc=s, L=L_true)


RECOVERY_GROUPS = ((1, 16), (2, 16), (128, 16), (129, 16), (300, 16), (3, 5))        # (frames, M)
NOISY = dict(n=129, L_true=2.7, seed=7, noise=1e-3, missing=5)
# Tolerances of the noisy case.  The central difference over 2 h = 2^-19 turns the points' rounding (about 2^-52 L) into an
# error of 2^-33 L in a Jacobian entry, hence about 2^-33 L rms sqrt(3 M) / a in an angle step: 1e-12 rad at 1 mm.  Every one
# of 129 frames' steps is never below the default 1e-12 at once, so the case runs at 1e-9 (rad, m), four orders below sigma_L.
NOISY_TOL = 1e-9
