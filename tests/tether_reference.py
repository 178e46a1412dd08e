"""50-digit reference of the tether keep-out cost of MPPI and CEM (law: include/rovmpc.h above rovmpc_set_tether_cost), the
plain fp64 NumPy restatement its margin is measured with, the error scale that ties the tolerance to each node's
conditioning, and the scenes both the host test and the GPU test run.

Everything takes the exact values a kernel holds: U and traj already rounded to the handle's dtype, the state in double.
The root, axes and rotation are those of tests/cable_reference.py.  tests/test_tether_reference_host.py measures the margin
M_TETHER below on the CPU and checks the scenes' conditions; tests/test_tether_gpu.py holds the kernel to the same bounds."""
import collections
import functools
import math

import numpy as np
from mpmath import mp, mpf

import cable_reference as cr

DPS = cr.DPS
EPS = cr.EPS
L_WS = cr.L_WS
BRACKET = cr.C_SHAPE                 # the engine bracket of the scenes: every root of the shape geometry inside
C_STEP = 1e-3 / 60.0                 # v_scale * dt of the default configuration, formed as the host forms it

# Margin: twice the largest ratio of the plain fp64 restatement's own error (tether_np against the 50-digit reference) to the
# scale below, over every scene, never below 4 -- the protocol of M_Z in cable_reference.py.
# Measured (test_tether_reference_host.py prints them): largest ratio 3.403 for a distance (N = 50, the path's fifty
# roundings), 0.070 for C_k; times 2, rounded up.
M_TETHER = 6.81

Ref = collections.namedtuple("Ref", "C D pen clear kappa rootC chord")


def _mp(x):
    return mpf(float(x))


def _rot_matrix(axis, c, s):
    """Rodrigues' rotation about the unit axis as a 3 x 3 list (cable_reference._rod written out as a matrix)."""
    x, y, z = axis
    o = 1 - c
    return [[c + x * x * o, x * y * o - z * s, x * z * o + y * s],
            [y * x * o + z * s, c + y * y * o, y * z * o - x * s],
            [z * x * o - y * s, z * y * o + x * s, c + z * z * o]]


def _matmul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _apply(m, v):
    return [m[i][0] * v[0] + m[i][1] * v[1] + m[i][2] * v[2] for i in range(3)]


def node_points(A, P, th, ga, L, M, up, c_lo, c_hi):
    """The M cable points of one node relative to A as mpf triples, the solve's kappa' (0 on the chord), its root C' (None:
    none) and whether the chord was used; None instead of the points where the node is non-finite.  A, P: mpf triples."""
    rel = [P[i] - A[i] for i in range(3)]
    if not (math.isfinite(th) and math.isfinite(ga)) or all(r == 0 for r in rel):
        return None, 0.0, None, False
    th, ga = _mp(th), _mp(ga)
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
    # both turns as one matrix: by -theta about the theta axis, then by gamma about the gamma axis
    R = _matmul(_rot_matrix(ga_axis, mp.cos(ga), mp.sin(ga)), _rot_matrix(th_axis, mp.cos(th), -mp.sin(th)))
    pts = []
    for m in range(M):
        t = mpf(m) / (M - 1)
        q = [t * Bp[0], t * Bp[1], up * (mp.cosh(C * (lp * t - x0)) - ch0) / C]
        pts.append(_apply(R, q))
    return pts, float(cr._kappa_mp(u, r, dHp, L)), C, False


def _seg_dist2_mp(a, b, c):
    e = [b[i] - a[i] for i in range(3)]
    p = [c[i] - a[i] for i in range(3)]
    den = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    t = (p[0] * e[0] + p[1] * e[1] + p[2] * e[2]) / den if den > 0 else mpf(0)
    t = min(max(t, mpf(0)), mpf(1))
    q = [p[i] - t * e[i] for i in range(3)]
    return q[0] * q[0] + q[1] * q[1] + q[2] * q[2]


def _seg_dist2_np(a, b, c):
    """Squared point-to-segment distances in fp64: a, b (S, 3) segment ends, c (3,)."""
    e, p = b - a, c - a
    den = np.sum(e * e, axis=1)
    with np.errstate(all="ignore"):
        t = np.where(den > 0, np.sum(p * e, axis=1) / np.where(den > 0, den, 1.0), 0.0)
    q = p - np.clip(t, 0.0, 1.0)[:, None] * e
    return np.sum(q * q, axis=1)


def cable_distance(pts, c, f=None):
    """min over the segments of the point-to-segment distance from c (mpf triple, relative to A like pts), at 50 digits.  A
    minimum is exact in any order: the segments whose fp64 distance is not within 1e-6 of the fp64 minimum cannot hold it
    (the fp64 distances of these scenes are good to 1e-12) and are not evaluated at 50 digits.  f: pts rounded to fp64."""
    if f is None:
        f = np.array([[float(x) for x in p] for p in pts])
    d2 = _seg_dist2_np(f[:-1], f[1:], np.array([float(x) for x in c]))
    d = np.sqrt(d2)
    near = np.nonzero(d <= d.min() + 1e-6)[0]
    return mp.sqrt(min(_seg_dist2_mp(pts[s], pts[s + 1], c) for s in near))


def tether_ref(state, U, traj, spheres, w, margin, L=L_WS, M=16, up=1.0, bracket=BRACKET, c=C_STEP):
    """The law at 50 digits for candidates U (K, N, 3) and stored angles traj (K, N + 1, 2).  Returns Ref: C (K mpf, or
    mp.inf), D (K, N) object array of mpf (mp.nan at a non-finite node), pen and clear = d - (R + margin) (K, N, J) object
    arrays, kappa' (K, N), the root C' (K, N; NaN: none) and the chord flags (K, N)."""
    U, traj, spheres = np.asarray(U), np.asarray(traj), np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    K, N, J = U.shape[0], U.shape[1], len(spheres)
    with mp.workdps(DPS):
        A = [_mp(x) for x in state[0:3]]
        Lm, upm, cm = _mp(L), _mp(up), _mp(c)
        c_lo, c_hi = _mp(bracket[0]), _mp(bracket[1])
        cen = [[_mp(s[i]) - A[i] for i in range(3)] for s in spheres]
        rm = [_mp(s[3]) + _mp(margin) for s in spheres]
        Cs = []
        D = np.empty((K, N), dtype=object); pen = np.empty((K, N, J), dtype=object); clear = np.empty((K, N, J), dtype=object)
        kap = np.zeros((K, N)); rootC = np.full((K, N), np.nan); chord = np.zeros((K, N), dtype=bool)
        for k in range(K):
            P = [_mp(x) for x in state[3:6]]
            Ck, bad = mpf(0), False
            for n in range(N):                                            # node n + 1 of the law
                P = [cm * _mp(U[k, n, ch]) + P[ch] for ch in range(3)]
                pts, kap[k, n], rc, chord[k, n] = node_points(A, P, float(traj[k, n + 1, 0]), float(traj[k, n + 1, 1]), Lm, M, upm, c_lo, c_hi)
                if rc is not None:
                    rootC[k, n] = float(rc)
                if pts is None:
                    bad = True
                    D[k, n] = mp.nan
                    pen[k, n, :] = mp.nan; clear[k, n, :] = mp.nan
                    continue
                f = np.array([[float(x) for x in p] for p in pts])
                for j in range(J):
                    d = cable_distance(pts, cen[j], f)
                    pen[k, n, j] = max(mpf(0), rm[j] - d)
                    clear[k, n, j] = d - rm[j]
                    Ck += _mp(w) * pen[k, n, j] ** 2
                D[k, n] = min(clear[k, n])
            Cs.append(mp.inf if bad else Ck)
    return Ref(Cs, D, pen, clear, kap, rootC, chord)


# ---- the plain fp64 restatement -----------------------------------------------------------------------------------------

def tether_np(state, U, traj, spheres, w, margin, L=L_WS, M=16, up=1.0, bracket=BRACKET, c=C_STEP):
    """The law in plain fp64 NumPy in the oracle's style (its axes, Rodrigues rotation and catenary solve, the samples of
    oracle.augmented_lowest_z_vec).  Returns (C (K,), D (K, N))."""
    from oracle import rovmpc_oracle as orc
    U = np.asarray(U, dtype=np.float64); traj = np.asarray(traj, dtype=np.float64)
    spheres = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    K, N, J = U.shape[0], U.shape[1], len(spheres)
    A = np.asarray(state[0:3], dtype=np.float64)
    P = np.tile(np.asarray(state[3:6], dtype=np.float64), (K, 1))
    Csum = np.zeros(K); bad = np.zeros(K, dtype=bool); D = np.empty((K, N))
    for n in range(N):
        P = c * U[:, n] + P
        rel = P - A
        th, ga = traj[:, n + 1, 0], traj[:, n + 1, 1]
        with np.errstate(all="ignore"):
            th_axis, ga_axis = orc._axes_vec(rel)
            Bp = orc._rod_vec(rel, th_axis, th)
            lp = np.sqrt(Bp[:, 0] ** 2 + Bp[:, 1] ** 2)
            dHp = up * Bp[:, 2]
            Cp = orc.solve_catenary_vec(lp, dHp, L, bracket[0], bracket[1])
            valid = np.isfinite(Cp)
            Cq = np.where(valid, Cp, 1.0)
            # cosh(C'(l' t - x0)) - cosh(C' x0) = 2 sinh(u' t) sinh(u' (t - 1) + atanh(dH'/L)) with u' = l' C' / 2: the same
            # value, without the difference of two cosh that a slack cable makes as large as e^u'
            uq = 0.5 * lp * Cq
            ath = np.arctanh(np.where(valid, dHp / L, 0.0))
            X = np.empty((K, M, 3))
            for m in range(M):
                t = m / (M - 1)
                q = np.stack([t * Bp[:, 0], t * Bp[:, 1], up * (2.0 * np.sinh(uq * t) * np.sinh(uq * (t - 1.0) + ath)) / Cq], axis=1)
                q = orc._rod_vec(orc._rod_vec(q, th_axis, -th), ga_axis, ga)
                X[:, m] = np.where(valid[:, None], q, t * rel)
            X = np.where((np.isfinite(th) & np.isfinite(ga) & np.isfinite(ga_axis).all(axis=1))[:, None, None], X, np.nan)
        fin = np.isfinite(X).all(axis=(1, 2))
        bad |= ~fin
        clear = np.full((K, J), np.nan)
        for k in np.nonzero(fin)[0]:
            for j in range(J):
                d = math.sqrt(_seg_dist2_np(X[k, :-1], X[k, 1:], spheres[j, :3] - A).min())
                rm = spheres[j, 3] + margin
                g = max(0.0, rm - d)
                Csum[k] += g * g
                clear[k, j] = d - rm
        D[:, n] = np.where(fin, clear.min(axis=1), np.nan)
    return np.where(bad, np.inf, w * Csum), D


# ---- error scale and bounds ---------------------------------------------------------------------------------------------

def scales(ref, state, spheres, L=L_WS):
    """s[k][n][j] = 2^-52 (1 + kappa'_n) (L + |A| + |c_j|): the point-to-segment distance is 1-Lipschitz in the points."""
    spheres = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    size = L + np.linalg.norm(state[0:3]) + np.linalg.norm(spheres[:, :3], axis=1)
    return EPS * (1.0 + ref.kappa)[:, :, None] * size[None, None, :]


def bounds(ref, state, spheres, w, L=L_WS, m=M_TETHER):
    """(bound_D (K, N), bound_C (K,)): m s of the node's worst sphere, and sum w (2 pen delta + delta^2) with delta = m s."""
    s = scales(ref, state, spheres, L)
    delta = m * s
    pen = np.array([[[0.0 if not mp.isfinite(p) else float(p) for p in row] for row in cand] for cand in ref.pen])
    return delta.max(axis=2), np.sum(w * (2.0 * pen * delta + delta * delta), axis=(1, 2))


def errors(C, D, ref):
    """|C - C_ref| (K,) and |D - D_ref| (K, N) as floats; inf where one side is non-finite and the other is not or differs
    in kind (a +inf C_ref wants +inf, a NaN D_ref wants NaN), 0 where both are."""
    eC = np.empty(len(ref.C)); eD = np.empty(ref.D.shape)
    for k, r in enumerate(ref.C):
        eC[k] = (0.0 if C[k] == np.inf else np.inf) if r == mp.inf else (float(abs(mpf(float(C[k])) - r)) if np.isfinite(C[k]) else np.inf)
    for idx, r in np.ndenumerate(ref.D):
        g = D[idx]
        eD[idx] = (0.0 if np.isnan(g) else np.inf) if mp.isnan(r) else (float(abs(mpf(float(g)) - r)) if np.isfinite(g) else np.inf)
    return eC, eD


def ratios(C, D, ref, state, spheres, w, L=L_WS):
    """Largest error-to-scale ratios (distance, C_k): the errors over the bounds at m = 1; 0 / 0 counts as 0."""
    eC, eD = errors(C, D, ref)
    bD, bC = bounds(ref, state, spheres, w, L, m=1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rD = np.where(eD == 0, 0.0, eD / bD); rC = np.where(eC == 0, 0.0, eC / bC)
    return float(rD.max()), float(rC.max())


def check_J(J_gpu, J_in, ref, bound_C, dtype):
    """J' = (T)((double) J + C) on the finite J: the largest |J'_gpu - (J + C_ref)| over bound_C + one ulp of T at J' (<= 1
    passes; a +inf C_ref wants +inf); a non-finite J must be left bit for bit (returns inf otherwise)."""
    J_gpu, J_in = np.asarray(J_gpu), np.asarray(J_in)
    worst = 0.0
    for k in range(len(J_in)):
        if not np.isfinite(J_in[k]):
            if J_gpu[k:k + 1].tobytes() != J_in[k:k + 1].tobytes():
                return np.inf
            continue
        if ref.C[k] == mp.inf:
            if J_gpu[k] != np.inf:
                return np.inf
            continue
        want = mpf(float(J_in[k])) + ref.C[k]
        allow = bound_C[k] + float(np.spacing(np.abs(np.asarray(float(want))).astype(dtype)))
        worst = max(worst, float(abs(mpf(float(J_gpu[k])) - want)) / allow)
    return worst


# ---- the scenes ---------------------------------------------------------------------------------------------------------

SHAPES = ((1, 1, 2), (2, 5, 3), (11, 67, 16), (20, 130, 17), (50, 9, 4))      # (N, K, M)
FRAMES_AT = (2, 5, 3)                # the shape both frames are run at
W, MARGIN = 1.0e3, 0.05
ANCHOR = np.array([0.25, -0.5, 0.75])
# (cx, cy, cz, R) relative to the anchor: the first contains it; the others sit among the connection vectors' mid-spans
SPHERES_REL = np.array([[0.1, 0.05, -0.1, 0.4], [0.9, 0.6, -0.5, 0.8], [-0.7, 0.9, 0.3, 0.7], [0.2, -1.0, -0.9, 0.9],
                        [-1.0, -0.6, 0.6, 0.8], [1.1, -0.4, 0.9, 0.7], [-0.2, 0.3, -1.3, 0.8], [0.6, 1.2, 1.0, 0.6]])

Scene = collections.namedtuple("Scene", "N K M up state U traj spheres")


@functools.lru_cache(maxsize=None)
def scene(N, K, M, up=1.0):
    """State, candidates and stored angles of one shape, every value exactly representable in float32 as well (an fp64 and an
    fp32 handle hold the same numbers, so one reference serves both).  The vehicle's path of candidate k visits the
    connection vectors of cable_reference.shape_geometry() in an order of its own: U[k][n] = (g_next - g_here) / c.  P1 hangs
    vertically below the anchor and the candidates with k % 4 == 0 first move along z only, so their node 1 has a vertical
    rel (degenerate xy projection).  (theta, gamma) come from cable_reference.ANGLES plus small random values."""
    rng = np.random.default_rng(1000 * N + 10 * K + M)
    g = np.array(cr.shape_geometry(L_WS))
    vertical = g[20]
    assert vertical[0] == 0.0 and vertical[1] == 0.0
    state = np.zeros(16)
    state[0:3] = ANCHOR
    state[3:6] = ANCHOR + vertical
    U = np.empty((K, N, 3)); traj = np.zeros((K, N + 1, 2))
    for k in range(K):
        here = vertical
        for n in range(N):
            if n == 0 and k % 4 == 0:
                nxt = np.array([0.0, 0.0, -0.7 - 0.05 * (k % 7)])
            else:
                i = (5 * k + 7 * n + 3) % len(g)
                # (not the vertical one: a path that returns to it ends some 1e-9 m beside the anchor's vertical, where the
                # theta axis hangs on the path's own rounding; the vertical case is node 1 above, exactly)
                nxt = g[i if i != 20 else 7] * (1.0 + 0.02 * rng.uniform(-1.0, 1.0))
            U[k, n] = (nxt - here) / C_STEP
            here = nxt
            traj[k, n + 1] = (cr.ANGLES[(k + 2 * n) % 5] + 0.01 * rng.standard_normal(), cr.ANGLES[(3 * k + n + 1) % 5] + 0.01 * rng.standard_normal())
    traj[:, 0] = (-0.0342, -0.0522)
    U = U.astype(np.float32).astype(np.float64)
    traj = traj.astype(np.float32).astype(np.float64)
    spheres = SPHERES_REL.copy()
    spheres[:, :3] += ANCHOR
    return Scene(N, K, M, up, state, U, traj, spheres)


@functools.lru_cache(maxsize=None)
def scene_reference(N, K, M, up=1.0):
    """(scene, Ref for all 8 spheres).  The spheres of a setting with fewer are the first ones, and C_k is added in node
    order, then sphere order, so `prefix` below gives their reference without another pass."""
    sc = scene(N, K, M, up)
    return sc, tether_ref(sc.state, sc.U, sc.traj, sc.spheres, W, MARGIN, M=M, up=up)


def prefix(ref, J):
    """The reference of the first J spheres from the reference of all of them."""
    with mp.workdps(DPS):
        K, N = ref.D.shape
        Cs = []
        D = np.empty((K, N), dtype=object)
        for k in range(K):
            Ck = mpf(0)
            for n in range(N):
                for j in range(J):
                    Ck += _mp(W) * ref.pen[k, n, j] ** 2
                D[k, n] = mp.nan if mp.isnan(ref.D[k, n]) else min(ref.clear[k, n, :J])
            Cs.append(mp.inf if ref.C[k] == mp.inf else Ck)
        return Ref(Cs, D, ref.pen[:, :, :J], ref.clear[:, :, :J], ref.kappa, ref.rootC, ref.chord)
