"""The navigation cost of MPPI / CEM (include/rovmpc.h, rovmpc_set_nav_cost) restated in 50-digit mpmath on the T-rounded
controls, and with each C_k a first-order running error bound for an evaluation of the law in double.

The bound is u = 2^-53 times, for every term of the sum, (the number of roundings on the term's path, its depth) x (the
term's magnitude with absolute values taken inside the differences), summed over the terms:

  P_n      = P_0 + c sum U_i           n roundings (one fma per node);       |P|_n = |P_0| + |c| sum |U_i|
  e_n      = P_n - ref                 n + 1;                                |e|_n = |P|_n + |ref|
  w e_n^2                              2 (n + 1) + 2 (square, weight) + S;   w |e|_n^2
  w_du (U_n - U_{n-1})^2               2 + 2 + S;                            w_du (|U_n| + |U_{n-1}|)^2
  d_nj     = |P_n - c_j|               n + 1 per component, + 5 (three squares and sums, the root);  |d|_nj = sum_ch (|P|_n + |c_j|)
  g_nj     = max(0, R_j - d_nj)        one more (max is 1-Lipschitz);        |g|_nj = R_j + |d|_nj
  w_s g^2                              2 (n + 7) + 2 + S;                    w_s |g|_nj^2

with S = N + n_spheres + 6 the additions a term can pass through on its way into C_k, in whatever order.  No tolerance is
fixed in advance: an implementation in double must lie within a small multiple of the bound (the tests allow 4x, for a
different association order and fma contraction)."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
U64 = 1 << 64
UNIT = 2.0 ** -53


def track_row(step, origin, n, Tr):
    """r(n) = clamp((int64)(step - origin) + n, 0, Tr - 1): the subtraction in uint64 (it wraps), then read as signed."""
    d = (int(step) - int(origin)) % U64
    if d >= 1 << 63:
        d -= U64
    return min(max(d + n, 0), Tr - 1)


def path(P1, U, c):
    """P_1 .. P_N (N, 3) as mpf lists for one candidate U (N, 3)."""
    P = [mp.mpf(float(v)) for v in P1]
    out = []
    for n in range(len(U)):
        P = [P[ch] + mp.mpf(c) * mp.mpf(float(U[n][ch])) for ch in range(3)]
        out.append(P)
    return out


def nav_cost_ref(P1, U, step, c, track, w_pos=(0, 0, 0), w_term=(0, 0, 0), w_du=(0, 0, 0), w_sphere=0.0, spheres=(), origin=0):
    """C_k of every candidate of U (K, N, 3) (an array of the handle's dtype: its values are taken exactly) against one track
    (Tr, 3).  Returns (C: list of K mpf, bound: (K,) float64)."""
    U = np.asarray(U)
    K, N = U.shape[:2]
    track = np.asarray(track, dtype=np.float64).reshape(-1, 3)
    Tr = len(track)
    spheres = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    wp, wt, wd = ([float(v) for v in np.broadcast_to(np.asarray(w, dtype=np.float64), (3,))] for w in (w_pos, w_term, w_du))
    ws = float(w_sphere)
    S = N + len(spheres) + 6
    rows = [track[track_row(step, origin, n, Tr)] for n in range(1, N + 1)]
    Cs, bounds = [], np.zeros(K)
    absP0 = np.abs(np.asarray(P1, dtype=np.float64))
    for k in range(K):
        Pk = path(P1, U[k], c)
        absU = np.abs(U[k].astype(np.float64))
        absP = absP0 + abs(c) * np.cumsum(absU, axis=0)            # (N, 3): |P|_n for n = 1 .. N
        Ck, bk = mp.mpf(0), 0.0
        for i in range(N):                                           # node n = i + 1
            n = i + 1
            for ch in range(3):
                e = Pk[i][ch] - mp.mpf(float(rows[i][ch]))
                mag = (absP[i][ch] + abs(rows[i][ch])) ** 2
                Ck += mp.mpf(wp[ch]) * e * e
                bk += (2 * (n + 1) + 2 + S) * wp[ch] * mag
                if n == N:
                    Ck += mp.mpf(wt[ch]) * e * e
                    bk += (2 * (n + 1) + 2 + S) * wt[ch] * mag
                if i >= 1:
                    d = mp.mpf(float(U[k][i][ch])) - mp.mpf(float(U[k][i - 1][ch]))
                    Ck += mp.mpf(wd[ch]) * d * d
                    bk += (4 + S) * wd[ch] * (absU[i][ch] + absU[i - 1][ch]) ** 2
            for sp in spheres:
                dist = mp.sqrt(sum((Pk[i][ch] - mp.mpf(float(sp[ch]))) ** 2 for ch in range(3)))
                g = max(mp.mpf(0), mp.mpf(float(sp[3])) - dist)
                Ck += mp.mpf(ws) * g * g
                bk += (2 * (n + 7) + 2 + S) * ws * (sp[3] + float(np.sum(absP[i] + np.abs(sp[:3])))) ** 2
        Cs.append(Ck)
        bounds[k] = UNIT * bk
    return Cs, bounds


def as_float(Cs):
    return np.array([float(v) for v in Cs], dtype=np.float64)


def ulp(x, dtype):
    """One unit in the last place of |x| in `dtype`."""
    return np.spacing(np.abs(np.asarray(x)).astype(dtype)).astype(np.float64)


def check_C(C_gpu, Cs, bounds, factor=4.0):
    """max ratio |C_gpu - C_ref| / bound over the candidates (0 / 0 counts as 0), and whether every candidate lies within
    factor x bound."""
    err = np.array([float(abs(mp.mpf(float(g)) - r)) for g, r in zip(C_gpu, Cs)])
    ok = bool(np.all(err <= factor * bounds))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bounds)
    return float(ratio.max()) if len(ratio) else 0.0, ok


def check_J(J_gpu, J_in, Cs, bounds, dtype, factor=4.0):
    """J' = (T)((double) J + C) on the finite J: the largest excess of |J'_gpu - (J + C_ref)| over factor x bound + one ulp of
    T at J', divided by that allowance (<= 1 passes); non-finite J must be left bit for bit."""
    J_gpu, J_in = np.asarray(J_gpu), np.asarray(J_in)
    worst = 0.0
    for k in range(len(J_in)):
        if not np.isfinite(J_in[k]):
            if J_gpu[k:k + 1].tobytes() != J_in[k:k + 1].tobytes():
                return np.inf
            continue
        ref = mp.mpf(float(J_in[k])) + Cs[k]
        allow = factor * bounds[k] + float(ulp(float(ref), dtype))
        worst = max(worst, float(abs(mp.mpf(float(J_gpu[k])) - ref)) / allow)
    return worst
