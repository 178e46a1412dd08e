"""50-digit references, deterministic workspaces and per-point bounds for the estimation kernels of csrc/util_kernels.h:
kabsch_kernel, gaussian_filter1d_kernel, features_dd_pass1_kernel (Savitzky-Golay), gradient_columns_kernel / np_gradient,
extract_features_kernel and replay_increments_kernel.  No GPU here: test_estimation_reference_host.py measures the margins on
the float64 oracle (numpy / scipy / oracle.*), test_estimation_kernels_gpu.py holds the kernels to them.

Every reference takes its float64 inputs as exact.  A 50-digit value x* is kept as the pair (hi, lo) = (float(x*),
float(x* - hi)), so |x - x*| = |(x - hi) - lo| is evaluated in float64 to ~1e-32.

Kabsch.  R* = V U^T of H = sum_i Pc_i Qc_i^T = U S V^T (mp.svd_r), last row of V^T negated when det < 0.  With
kappa = (sum_i |p_i| |q_i|) / (sigma_2 + d sigma_3), d = sign det(V U^T), the uncentred norms in the numerator (so the
cancellation of the centring is covered):   |R - R*|_max <= m_R eps (1 + kappa),
|v_out - R* v|_max <= (m_R eps (1 + kappa) + 4 eps) |v|_1.   A frame with eps kappa > 1e-3 is undecided.

Sums (FIR taps, np.gradient, the feature map's quotients): scale = eps (sum of |term| over the terms actually added + |sum|),
bound = m * scale; np.gradient's middle coefficient enters the scale as (|dx1| + |dx2|) / (dx1 dx2).  A chained gradient pass adds
the previous pass's bound carried through the absolute values of the same coefficients."""
import functools
import math
from collections import namedtuple

import numpy as np
from mpmath import mp, mpf

DPS = 50
EPS = 2.0 ** -52
UNDECIDED = 1e-3                    # eps * kappa above this: the frame is compared with nothing
MS = (3, 4, 16, 17, 64)
N_FRAMES = 257                      # per M: two full 128-lane blocks and a third block of one lane


def split(x):
    hi = float(x)
    return hi, float(x - mpf(hi))


def err(x, hi, lo):
    """|x - x*| elementwise, x* = hi + lo."""
    return np.abs((np.asarray(x, np.float64) - hi) - lo)


# ---- Kabsch ---------------------------------------------------------------------------------------------------------------

Frame = namedtuple("Frame", "family tag P Q v gen")


def rotation(axis, ang):
    k = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


PERMS = (np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]),
         np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]]), np.array([[0.0, 0, 1], [0, -1, 0], [1, 0, 0]]))   # exact, det +1


def _isotropic_sets(M):
    """Marker sets with equal (non-zero) singular values of Pc^T Pc, padded to M with points at the centroid."""
    tri = [[1.0, 0, 0], [-0.5, 0.75 ** 0.5, 0], [-0.5, -(0.75 ** 0.5), 0]]
    square = [[1.0, 1, 0], [-1, 1, 0], [-1, -1, 0], [1, -1, 0]]
    tetra = [[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]
    octa = [[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    cube = [[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]
    sets = {3: [("triangle", tri)], 4: [("square", square), ("tetrahedron", tetra)]}.get(
        M, [("octahedron", octa), ("square", square), ("octahedron+cube", octa + cube)])
    return [(n, np.array(p + [[0.0, 0, 0]] * (M - len(p)))) for n, p in sets]


@functools.lru_cache(maxsize=None)
def kabsch_workspace(M):
    """N_FRAMES frames of M markers; every family (a)-(g) of the module's users is present for every M."""
    rng = np.random.default_rng(7100 + M)
    fr = []

    def generic(ang, noise=1e-3):
        P = rng.normal(size=(M, 3)) * 0.5 + rng.normal(size=3)
        R = rotation(rng.normal(size=3), ang)
        return P, P @ R.T + rng.normal(size=3) * 0.3 + noise * rng.normal(size=(M, 3))

    def add(family, tag, P, Q, gen=False):
        fr.append(Frame(family, tag, np.ascontiguousarray(P, np.float64), np.ascontiguousarray(Q, np.float64), rng.normal(size=3) * 0.3, gen))

    # (a) generic markers, rotation angles 0 .. pi inclusive
    a_frames = []
    for ang in np.linspace(0.0, math.pi, 17):
        P, Q = generic(float(ang))
        a_frames.append((ang, P, Q))
        add("a", "angle=%.4f" % ang, P, Q)
    # (b) cable-like: a sagging curve in a vertical plane, slightly out of plane, mm with offsets up to 1e4; and in metres
    for j in range(10):
        s = np.linspace(-1.0, 1.0, M) * rng.uniform(800.0, 1400.0)
        a = rng.uniform(900.0, 2500.0)
        psi = rng.uniform(0, 2 * math.pi)
        P = (rng.uniform(-1e4, 1e4, size=3) + np.outer(s, [math.cos(psi), math.sin(psi), 0.0]) + np.outer(a * (np.cosh(s / a) - 1), [0, 0, 1.0])
             + np.outer(rng.normal(size=M), [-math.sin(psi), math.cos(psi), 0.0]))
        c = P.mean(axis=0)
        Q = (P - c) @ rotation(rng.normal(size=3), rng.uniform(0.0, 0.3)).T + c + rng.normal(size=3) * 20 + 0.5 * rng.normal(size=(M, 3))
        add("b", "mm %d" % j, P, Q)
        add("b", "m %d" % j, P / 1000, Q / 1000)
    # (c) exactly planar sets, exact rotations, P == Q
    for j in range(2):
        Pp = rng.normal(size=(M, 3)) * 0.5 + rng.normal(size=3); Pp[:, 2] = 0.25
        Pg = rng.normal(size=(M, 3)) * 0.5 + rng.normal(size=3)
        add("c", "planar, exact 90 deg about z", Pp, Pp @ PERMS[1].T)
        add("c", "planar, exact 180 deg about x", Pp, Pp @ PERMS[2].T)
        add("c", "planar, generic rotation", Pp, Pp @ rotation(rng.normal(size=3), 1.1).T)
        add("c", "planar, in-plane noise", Pp, Pp + np.hstack([1e-3 * rng.normal(size=(M, 2)), np.zeros((M, 1))]))
        add("c", "generic, exact cyclic permutation", Pg, Pg @ PERMS[0].T)
        add("c", "generic, exact 180 deg about x", Pg, Pg @ PERMS[2].T)
        add("c", "P == Q generic", Pg, Pg.copy())
        add("c", "P == Q planar", Pp, Pp.copy())
    # (d) mirrored sets, d = -1: Pc = A diag(1, s2, s3) G^T with orthonormal centred columns A, so H has the singular values
    #     (1, s2^2, s3^2); three markers span a plane and have sigma_3 = 0 whatever the ratio asked for
    s2 = 0.7
    for tag, ratio in [("0.5", 0.5), ("1e-3", 1e-3), ("1e-6", 1e-6)] * 2 + [("sigma2~sigma3", 1 - 1e-6)]:
        X = rng.normal(size=(M, 3)); X -= X.mean(axis=0)
        A = np.linalg.svd(X, full_matrices=False)[0]
        S = np.diag([1.0, s2, s2 * math.sqrt(ratio) if M > 3 else 0.0])
        G = rotation(rng.normal(size=3), 0.9)
        P = A @ S @ G.T + rng.normal(size=3)
        Q = A @ S @ np.diag([1.0, 1.0, -1.0]) @ G.T @ rotation(rng.normal(size=3), 0.7).T + rng.normal(size=3)
        add("d", tag, P, Q)
    # (e) equal singular values under generic and axis-permuting rotations
    for name, P0 in _isotropic_sets(M):
        off = rng.integers(-3, 4, size=3).astype(float)
        add("e", name + ", generic rotation", P0 + off, P0 @ rotation(rng.normal(size=3), 0.8).T + off)
        add("e", name + ", generic rotation, noise", P0 + off, P0 @ rotation(rng.normal(size=3), 2.0).T + 1e-3 * rng.normal(size=(M, 3)))
        for k in (0, 1, 3):
            add("e", name + ", permutation %d" % k, P0 + off, P0 @ PERMS[k].T - off)
    # (f) near-collinear: transverse extent eps of the length
    for tag, e in [("1e-3", 1e-3), ("1e-6", 1e-6), ("1e-9", 1e-9), ("1e-12", 1e-12)] * 2:
        d = rotation(rng.normal(size=3), 1.3)
        s = np.linspace(-1.0, 1.0, M) + 0.1 * rng.normal(size=M)
        P = np.outer(s, d[0]) + e * (np.outer(rng.normal(size=M), d[1]) + np.outer(rng.normal(size=M), d[2]))
        add("f", tag, P, P @ rotation(rng.normal(size=3), 0.5).T + 0.1 * rng.normal(size=3))
    #     exactly collinear (a rank-one H: no rotation is determined): integer multiples of integer directions with integer
    #     offsets, so P and the axis-permuted Q are collinear in float64 itself; times 3 and 1000 likewise, times 0.1 and 1.7
    #     collinear to an ulp
    sc = np.arange(M, dtype=float) - (M // 2)
    for j, dirn in enumerate(([1.0, 2.0, -2.0], [1.0, 0.0, 0.0], [3.0, -1.0, 2.0], [1.0, 1.0, 1.0], [0.0, 2.0, 5.0])):
        for mult in (1.0, 3.0, 0.1, 1.7, 1000.0):
            Pl = (np.outer(sc, dirn) + rng.integers(-4, 5, size=3).astype(float)) * mult
            add("f", "collinear, exact rotation, direction %d x %g" % (j, mult), Pl, Pl @ PERMS[j % 4].T)
            add("f", "collinear, generic rotation, direction %d x %g" % (j, mult), Pl, Pl @ rotation(rng.normal(size=3), 0.5).T + mult * rng.normal(size=3))
    # (g) family (a) scaled by 2^(+-k): every other angle, 0 and pi included
    for k in (10, 100, 400):
        for sgn in (1, -1):
            for ang, P, Q in a_frames[::2]:
                add("g", "k=%+d" % (sgn * k), np.ldexp(P, sgn * k), np.ldexp(Q, sgn * k))
    # more of (a), random angles, up to the frame count
    while len(fr) < N_FRAMES:
        P, Q = generic(rng.uniform(0.0, math.pi))
        add("a", "fill", P, Q)
    assert len(fr) == N_FRAMES and N_FRAMES % 128 == 1
    return tuple(fr)


KabschTruth = namedtuple("KabschTruth", "R v sigma d kappa")


def kabsch_true(P, Q, v):
    """(R*, R* v, (sigma_1, sigma_2, sigma_3), d, kappa) at DPS digits; R*, v* as mp matrices."""
    with mp.workdps(DPS):
        M = len(P)
        Pm = [[mpf(float(x)) for x in r] for r in P]; Qm = [[mpf(float(x)) for x in r] for r in Q]
        cp = [mp.fsum(r[a] for r in Pm) / M for a in range(3)]; cq = [mp.fsum(r[a] for r in Qm) / M for a in range(3)]
        H = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                H[a, b] = mp.fsum((Pm[i][a] - cp[a]) * (Qm[i][b] - cq[b]) for i in range(M))
        U, S, Vt = mp.svd_r(H)
        R = Vt.T * U.T
        d = 1 if mp.det(R) >= 0 else -1
        if d < 0:
            for b in range(3):
                Vt[2, b] = -Vt[2, b]
            R = Vt.T * U.T
        num = mp.fsum(mp.sqrt(mp.fsum(x * x for x in p)) * mp.sqrt(mp.fsum(x * x for x in q)) for p, q in zip(Pm, Qm))
        den = S[1] + d * S[2]
        kappa = float(num / den) if den > 0 else math.inf
        return KabschTruth(R, R * mp.matrix([mpf(float(x)) for x in v]), tuple(float(S[j]) for j in range(3)), d, kappa)


KabschTable = namedtuple("KabschTable", "frames P Q v R_hi R_lo w_hi w_lo sigma d kappa decided")


@functools.lru_cache(maxsize=None)
def kabsch_table(M):
    fr = kabsch_workspace(M)
    T = len(fr)
    R_hi = np.empty((T, 3, 3)); R_lo = np.empty((T, 3, 3)); w_hi = np.empty((T, 3)); w_lo = np.empty((T, 3))
    sigma = np.empty((T, 3)); d = np.empty(T, int); kappa = np.empty(T)
    for t, f in enumerate(fr):
        tr = kabsch_true(f.P, f.Q, f.v)
        with mp.workdps(DPS):
            for a in range(3):
                w_hi[t, a], w_lo[t, a] = split(tr.v[a])
                for b in range(3):
                    R_hi[t, a, b], R_lo[t, a, b] = split(tr.R[a, b])
        sigma[t] = tr.sigma; d[t] = tr.d; kappa[t] = tr.kappa
    for x in (R_hi, R_lo, w_hi, w_lo, sigma, d, kappa):
        x.setflags(write=False)
    return KabschTable(fr, np.stack([f.P for f in fr]), np.stack([f.Q for f in fr]), np.stack([f.v for f in fr]), R_hi, R_lo, w_hi, w_lo,
                       sigma, d, kappa, EPS * kappa <= UNDECIDED)


def kabsch_bounds(t, m_R):
    """(bound on |R - R*|_max, bound on |v_out - R* v|_max) per frame."""
    bR = m_R * EPS * (1 + t.kappa)
    return bR, (bR + 4 * EPS) * np.abs(t.v).sum(axis=1)


def kabsch_errors(t, R, v_out, idx=None):
    """(|R - R*|_max, |v_out - R* v|_max) per frame of idx (default: all)."""
    s = slice(None) if idx is None else idx
    return err(R, t.R_hi[s], t.R_lo[s]).max(axis=(1, 2)), err(v_out, t.w_hi[s], t.w_lo[s]).max(axis=1)


def orthogonality_defect(R):
    R = np.asarray(R, np.float64)
    return np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max(axis=(-1, -2))


# ---- sums: helpers --------------------------------------------------------------------------------------------------------

Ref = namedtuple("Ref", "hi lo scale")          # x* = hi + lo; bound = m * scale (+ what a chain carries in)


def _acc(terms, extra_abs=None):
    """(sum, eps (sum |term| + |sum|)) of mp terms; extra_abs replaces sum |term| where a coefficient's own form asks for it."""
    s = mp.fsum(terms)
    return s, EPS * ((mp.fsum(abs(x) for x in terms) if extra_abs is None else extra_abs) + abs(s))


def _pack(vals, scales):
    hi = np.empty(len(vals)); lo = np.empty(len(vals))
    for i, x in enumerate(vals):
        hi[i], lo[i] = split(x)
    return Ref(hi, lo, np.array([float(s) for s in scales]))


def signal(T, seed, amp=0.3):
    """An angle-like series: slow waves, noise and a few spikes."""
    rng = np.random.default_rng(seed)
    i = np.arange(T)
    x = amp * np.sin(0.07 * i + rng.uniform(0, 6)) + 0.1 * np.cos(0.31 * i) + 0.02 * rng.normal(size=T)
    x[rng.integers(0, T, size=max(1, T // 40))] += rng.normal(size=max(1, T // 40))
    return x


def times(T, kind, seed):
    """Sample times: 'uniform' (0.02 s from an offset) or 'jitter' (steps between 2e-3 and 0.2 s, neighbours up to 100 apart in ratio)."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return 12.5 + 0.02 * np.arange(T)
    dt = 2e-3 * 100.0 ** rng.uniform(0, 1, size=T)
    dt[1::7] = 2e-3; dt[2::7] = 0.2            # the extreme ratio itself, next to each other
    return 3.0 + np.cumsum(dt)


# ---- Gaussian filter (scipy.ndimage.gaussian_filter1d, mode='reflect', truncate 4) ------------------------------------------

GAUSS_CASES = tuple((T, 2.0) for T in (1, 6, 255, 256, 257, 513)) + ((6, 3.5),)


def gaussian_weights(sigma, truncate=4.0):
    """w[0 .. radius] as rovmpc_gaussian_filter1d builds them on the host, statement by statement."""
    radius = int(truncate * sigma + 0.5)
    s = 0.0
    for k in range(-radius, radius + 1):
        s += math.exp(-0.5 / (sigma * sigma) * float(k) * float(k))
    return [math.exp(-0.5 / (sigma * sigma) * float(k) * float(k)) / s for k in range(radius + 1)]


def reflect(j, T):
    while j < 0 or j >= T:                       # d c b a | a b c d | d c b a, as often as needed
        j = -j - 1 if j < 0 else 2 * T - j - 1
    return j


def gaussian_reference(x, sigma):
    w = gaussian_weights(sigma)
    T = len(x)
    with mp.workdps(DPS):
        xm = [mpf(float(v)) for v in x]; wm = [mpf(v) for v in w]
        out = []
        for i in range(T):
            terms = [wm[0] * xm[i]]
            for k in range(1, len(w)):
                terms += [wm[k] * xm[reflect(i - k, T)], wm[k] * xm[reflect(i + k, T)]]
            out.append(_acc(terms))
        return _pack([o[0] for o in out], [o[1] for o in out])


# ---- Savitzky-Golay (scipy.signal.savgol_filter, mode='interp') -------------------------------------------------------------

SAVGOL_CASES = tuple((T, 11, 3) for T in (11, 12, 255, 256, 257, 513)) + ((21, 21, 5), (257, 21, 5))


@functools.lru_cache(maxsize=None)
def savgol_hat(window, order):
    """The window x window float64 hat matrix as rovmpc_features_dd builds it on the host (extended-precision monomials,
    modified Gram-Schmidt twice, H = Q Q^T), statement by statement."""
    ld = np.longdouble
    w, m, half = window, order + 1, window // 2
    Q = np.zeros((w, m), dtype=ld)
    for c in range(m):
        for r in range(w):
            Q[r, c] = ld(r - half) ** c if c else ld(1)
        for _ in range(2):
            for p in range(c):
                d = ld(0)
                for r in range(w):
                    d += Q[r, c] * Q[r, p]
                for r in range(w):
                    Q[r, c] -= d * Q[r, p]
        n = ld(0)
        for r in range(w):
            n += Q[r, c] * Q[r, c]
        n = np.sqrt(n)
        for r in range(w):
            Q[r, c] /= n
    H = np.empty((w, w))
    for i in range(w):
        for j in range(w):
            s = ld(0)
            for c in range(m):
                s += Q[i, c] * Q[j, c]
            H[i, j] = float(s)
    H.setflags(write=False)
    return H


def savgol_hat_exact(window, order):
    """The same projector from exact rational arithmetic (Gram matrix of the monomials), rounded once."""
    from fractions import Fraction
    w, m, half = window, order + 1, window // 2
    A = [[Fraction(r - half) ** c for c in range(m)] for r in range(w)]
    G = [[sum(A[r][a] * A[r][b] for r in range(w)) for b in range(m)] for a in range(m)]
    n = m                                           # G^-1 by Gauss-Jordan
    aug = [row[:] + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(G)]
    for c in range(n):
        p = next(r for r in range(c, n) if aug[r][c] != 0)
        aug[c], aug[p] = aug[p], aug[c]
        aug[c] = [x / aug[c][c] for x in aug[c]]
        for r in range(n):
            if r != c and aug[r][c] != 0:
                aug[r] = [x - aug[r][c] * y for x, y in zip(aug[r], aug[c])]
    Gi = [row[n:] for row in aug]
    return np.array([[float(sum(A[i][a] * Gi[a][b] * A[j][b] for a in range(m) for b in range(m))) for j in range(w)] for i in range(w)])


def _savgol_mp(xm, window, order):
    W = savgol_hat(window, order)
    T, half = len(xm), window // 2
    out = []
    for i in range(T):
        if i < half:
            first, row = 0, i
        elif i >= T - half:
            first, row = T - window, i - (T - window)
        else:
            first, row = i - half, half
        out.append(_acc([mpf(float(W[row, j])) * xm[first + j] for j in range(window)]))
    return out


def savgol_reference(x, window, order):
    with mp.workdps(DPS):
        out = _savgol_mp([mpf(float(v)) for v in x], window, order)
        return _pack([o[0] for o in out], [o[1] for o in out])


# ---- np.gradient (second-order non-uniform interior, first-order one-sided ends) ----------------------------------------------

GRAD_TS = (2, 3, 256, 257, 513)
Grad = namedtuple("Grad", "ref idx cabs vals")       # ref; rows read (T,3) and |coefficient| on each (T,3), to carry a bound through


def _gradient_mp(fm, tm):
    T = len(fm)
    vals, scales, idx, cabs = [], [], np.zeros((T, 3), int), np.zeros((T, 3))
    for i in range(T):
        if i == 0 or i == T - 1:
            j0, j1 = (0, 1) if i == 0 else (T - 2, T - 1)
            dt = tm[j1] - tm[j0]
            s, sc = _acc([fm[j1] / dt, -fm[j0] / dt])
            idx[i] = (j0, j1, j1); cabs[i] = (float(abs(1 / dt)), float(abs(1 / dt)), 0.0)
        else:
            dx1, dx2 = tm[i] - tm[i - 1], tm[i + 1] - tm[i]
            a, b, c = -dx2 / (dx1 * (dx1 + dx2)), (dx2 - dx1) / (dx1 * dx2), dx1 / (dx2 * (dx1 + dx2))
            terms = [a * fm[i - 1], b * fm[i], c * fm[i + 1]]
            wide = abs(terms[0]) + (abs(dx1) + abs(dx2)) / abs(dx1 * dx2) * abs(fm[i]) + abs(terms[2])
            s, sc = _acc(terms, wide)
            idx[i] = (i - 1, i, i + 1); cabs[i] = (float(abs(a)), float(abs(b)), float(abs(c)))
        vals.append(s); scales.append(sc)
    return vals, scales, idx, cabs


def gradient_reference(f, t):
    with mp.workdps(DPS):
        vals, scales, idx, cabs = _gradient_mp([mpf(float(v)) for v in f], [mpf(float(v)) for v in t])
        return Grad(_pack(vals, scales), idx, cabs, vals)


def carry(g, b):
    """The bound b on a gradient pass's input, carried to its output through the absolute coefficients."""
    return (g.cabs * np.asarray(b)[g.idx]).sum(axis=1)


Chain = namedtuple("Chain", "smooth d1 d2")          # Savitzky-Golay column, its gradient, the gradient of that (each a Ref / Grad)


def derivative_chain(x, t, window=11, order=3):
    """theta -> Savitzky-Golay -> np.gradient -> np.gradient at DPS digits throughout (compute_derivatives, and columns
    0/1, 2/3 and the targets of features_dd)."""
    with mp.workdps(DPS):
        tm = [mpf(float(v)) for v in t]
        sg = _savgol_mp([mpf(float(v)) for v in x], window, order)
        sm = [o[0] for o in sg]
        v1, s1, i1, c1 = _gradient_mp(sm, tm)
        v2, s2, i2, c2 = _gradient_mp(v1, tm)
        return Chain(_pack(sm, [o[1] for o in sg]), Grad(_pack(v1, s1), i1, c1, None), Grad(_pack(v2, s2), i2, c2, None))


def chain_bounds(ch, m_sg, m_grad):
    """Bounds of the three stages: each pass's own m * scale plus the previous stage's bound carried through."""
    b0 = m_sg * ch.smooth.scale
    b1 = m_grad * ch.d1.ref.scale + carry(ch.d1, b0)
    b2 = m_grad * ch.d2.ref.scale + carry(ch.d2, b1)
    return b0, b1, b2


# ---- extract_features (simply.py:15-41): the 16 / 18-column map ---------------------------------------------------------------

FEATURE_TS = (2, 255, 256, 257, 513)
EXACT_COLS = (0, 1, 2, 3, 4, 5, 14, 15, 16, 17)      # copies: bit-equal


def feature_inputs(T, seed=None):
    """(P0, P1, V1, time, theta, gamma) with rows where P1 == P0, V1 = 0, the cable length is clipped at both ends and the
    cosine at +-1 (placed at the block edges too when T allows)."""
    rng = np.random.default_rng(5200 + T if seed is None else seed)
    P0 = rng.normal(size=(T, 3)) * 0.3
    rel = rng.normal(size=(T, 3))
    rel *= (rng.uniform(0.5, 3.0, size=T) / np.linalg.norm(rel, axis=1))[:, None]
    V1 = rng.normal(size=(T, 3)) * 0.2
    special = sorted({0, 1, 2, T // 2, T - 3, T - 2, T - 1, 254, 255, 256, 257, 511, 512} & set(range(T)))
    for k, i in enumerate(special):
        kind = k % 6
        if kind == 0:
            rel[i] = 0.0                                                  # P1 == P0: the +1e-8 guard alone, length clipped at 1e-5
        elif kind == 1:
            V1[i] = 0.0
        elif kind == 2:
            rel[i] *= 12.0 / np.linalg.norm(rel[i])                       # clipped at 10
        elif kind == 3:
            rel[i] *= 3e-6 / np.linalg.norm(rel[i])                       # clipped at 1e-5
        else:                                                             # cosine beyond +-1 before the clip: both guards are below an
            while True:                                                   # ulp here, and the direction is drawn until float64 rounds over
                r = rng.normal(size=3) * 1e9
                nrm = np.linalg.norm(r[None], axis=1)[0] + 1e-8
                if np.sum(r * (r / nrm)) / nrm > 1.0:
                    break
            rel[i] = r
            P0[i] = 0.0
            V1[i] = r if kind == 4 else -r
    P1 = P0 + rel
    t = times(T, "jitter", 5300 + T)
    return P0, P1, V1, t, signal(T, 5400 + T), signal(T, 5500 + T, 0.2)


def features_reference(P0, P1, V1, time, theta, gamma):
    """(hi, lo, scale) of shape (T, 18); scale is 0 on the columns that are copies."""
    T = len(time)
    hi = np.zeros((T, 18)); lo = np.zeros((T, 18)); scale = np.zeros((T, 18))
    hi[:, 0:3] = P1; hi[:, 3:6] = V1; hi[:, 14] = theta; hi[:, 15] = gamma
    hi[:, 16] = np.concatenate([theta[:1], theta[:-1]]); hi[:, 17] = np.concatenate([gamma[:1], gamma[:-1]])
    for a in range(3):
        g = gradient_reference(V1[:, a], time).ref
        hi[:, 6 + a], lo[:, 6 + a], scale[:, 6 + a] = g.hi, g.lo, g.scale
    with mp.workdps(DPS):
        guard = mpf(1e-8)
        for i in range(T):
            r = [mpf(float(P1[i, a])) - mpf(float(P0[i, a])) for a in range(3)]
            v = [mpf(float(x)) for x in V1[i]]
            nr = mp.sqrt(mp.fsum(x * x for x in r))
            u = [x / (nr + guard) for x in r]
            nv = mp.sqrt(mp.fsum(x * x for x in v)) + guard
            cols = [(9 + a, u[a], 2 * EPS * abs(u[a])) for a in range(3)]
            cols.append((12, min(max(nr, mpf(1e-5)), mpf(10.0)), 2 * EPS * nr))
            c, sc = _acc([v[a] * u[a] / nv for a in range(3)])
            cols.append((13, min(max(c, mpf(-1)), mpf(1)), sc))
            for k, x, s in cols:
                hi[i, k], lo[i, k] = split(x)
                scale[i, k] = float(s)
    return Ref(hi, lo, scale)


# ---- v_sway, v_surge of features_dd (main_fun.py:839-843) -----------------------------------------------------------------------

def surge_sway_reference(P0_mm, P1_mm, V_mm):
    """(sway, surge) per row.  The quotients by 1000 are single correctly rounded operations and are taken in float64 (the V
    columns of the output are compared with them bit for bit); everything after them is at DPS digits: unit = rel / (|rel| +
    1e-8), surge = V . unit, sway = |V x unit| with scale eps (sum of the |products| entering the cross product + |sway|)."""
    p0, p1, vv = np.asarray(P0_mm) / 1000, np.asarray(P1_mm) / 1000, np.asarray(V_mm) / 1000
    sway, surge = [], []
    with mp.workdps(DPS):
        guard = mpf(1e-8)
        for i in range(len(vv)):
            r = [mpf(float(p1[i, a])) - mpf(float(p0[i, a])) for a in range(3)]
            v = [mpf(float(x)) for x in vv[i]]
            nr = mp.sqrt(mp.fsum(x * x for x in r)) + guard
            u = [x / nr for x in r]
            surge.append(_acc([v[a] * u[a] for a in range(3)]))
            c = [v[1] * u[2] - v[2] * u[1], v[2] * u[0] - v[0] * u[2], v[0] * u[1] - v[1] * u[0]]
            prods = abs(v[1] * u[2]) + abs(v[2] * u[1]) + abs(v[2] * u[0]) + abs(v[0] * u[2]) + abs(v[0] * u[1]) + abs(v[1] * u[0])
            sw = mp.sqrt(mp.fsum(x * x for x in c))
            sway.append((sw, EPS * (prods + sw)))
        return _pack([x[0] for x in sway], [x[1] for x in sway]), _pack([x[0] for x in surge], [x[1] for x in surge])


# ---- replay increments ------------------------------------------------------------------------------------------------------

REPLAY_TS = (2, 128, 129, 130, 257)
REPLAY_RTOL = 1e-11                                   # test_replay_integrators' tolerance against the oracle's float64 replay


def replay_rows(Xs, time, T):
    """T rows of a recorded log, repeated from its start (with its own time steps) where T is longer than the log."""
    n = len(time)
    t = np.asarray(time, np.float64)[:T]
    if T > n:
        t = np.concatenate([t, t[-1] + np.cumsum(np.diff(time)[np.arange(T - n) % (n - 1)])])
    return np.ascontiguousarray(Xs[np.arange(T) % n]), np.ascontiguousarray(t)
