"""50-digit reference of the cable chain (catenary root, tension, lowest point of the augmented shape), the
deterministic point set it is checked on, and the per-point bounds that tie a tolerance to the problem's conditioning.

Everything takes the exact doubles a kernel receives.  tests/test_cable_reference_host.py measures the margins below on
the CPU and checks the reference itself; tests/test_cable_geometry_gpu.py holds the kernels to the same bounds."""
import collections
import functools
import math

import numpy as np
from mpmath import mp, mpf

DPS = 50
EPS = 2.0 ** -52
EPS32 = 2.0 ** -23
XTOL = 2e-12                    # scipy brentq's documented default xtol: the plain fp64 reference is no better than this
L_WS = 3.0
W_WET = 1.521                   # cable_wet_weight of the default configuration
C_NARROW = (0.5, 4.0)           # family (c): both bracket ends where kappa * eps is small
C_WIDE = (1e-6, 1e10)           # every root of the workspace inside the bracket
C_DEFAULT = (1e-6, 10.0)        # the bracket of rv.solve_catenary / rv.cable_tension
C_SHAPE = (1e-6, 200.0)         # lowest-point cases: every root inside, and the oracle's f(c_hi) ~ sinh^2(l c_hi / 2) still finite
LS = (0.05, 0.3, 1.0, 2.5, 2.99)

# Margins: twice the largest ratio of the plain fp64 reference's own error to the conditioning scale
# (test_cable_reference_host.py measures them and fails if the reference leaves m / 2), never below 4.
M_C = 4.0                       # measured: largest ratio 0.258 for C (brentq), 2 * 0.258 < 4
M_T = 4.0                       # measured: largest ratio 0.258 for the tension, 2 * 0.258 < 4
M_Z = 6.07                      # measured: largest ratio 3.031 for the lowest point (oracle against 50 digits), times 2, rounded up

Point = collections.namedtuple("Point", "family tag l dH L")


def _mp(x):
    return mpf(float(x))


# ---- root ---------------------------------------------------------------------------------------------------------

def _root_mp(l, dH, L):
    """(u*, C*, r) as mpf for mpf inputs, or None: positive root of sinh(u) = r u, r = sqrt(L^2 - dH^2) / l."""
    for v in (l, dH, L):
        if not mp.isfinite(v):
            return None
    if not (l > 0 and L > 0):
        return None
    with mp.workdps(DPS + 25):
        L2 = L * L - dH * dH
        if L2 <= l * l:
            return None
        r = mp.sqrt(L2) / l
        # series start: root of y/6 + y^2/120 = r - 1 in y = u^2, an upper bound of the root (sinh u / u >= 1 + u^2/6 + u^4/120);
        # h(u) = sinh u - r u is convex right of its root, so Newton from there descends monotonically
        rm1 = (L2 - l * l) / (l * (mp.sqrt(L2) + l))
        u = mp.sqrt(60 * (mp.sqrt(mpf(1) / 36 + rm1 / 30) - mpf(1) / 6))
        if r > 8:
            ul = mp.log(2 * r * u)
            for _ in range(3):
                ul = mp.log(2 * r * ul)
            ul = ul * (1 + mpf(1) / 64)
            if mp.sinh(ul) > r * ul and ul < u:
                u = ul
        tiny = mpf(10) ** -(DPS - 5)             # quadratic convergence: the step after this one is below 1e-80
        for _ in range(200):
            d = (mp.sinh(u) - r * u) / (mp.cosh(u) - r)
            u = u - d
            if abs(d) < tiny * u:
                break
        else:
            raise RuntimeError("reference root did not converge")
        u = u - (mp.sinh(u) - r * u) / (mp.cosh(u) - r)
        return +u, 2 * u / l, r


@functools.lru_cache(maxsize=None)
def _root_cached(l, dH, L):
    with mp.workdps(DPS):
        return _root_mp(mpf(l), mpf(dH), mpf(L))


def true_root(l, dH, L):
    """(u*, C*) at 50 digits for the doubles (l, dH, L), or None when L^2 - dH^2 <= l^2 or an input is non-finite / non-positive."""
    l, dH, L = float(l), float(dH), float(L)
    if not (math.isfinite(l) and math.isfinite(dH) and math.isfinite(L)):
        return None
    r = _root_cached(l, dH, L)
    return None if r is None else (r[0], r[1])


def _kappa_mp(u, r, dH, L):
    L2 = L * L - dH * dH
    return r / (mp.cosh(u) - r) * (1 + (L * L + dH * dH) / (2 * L2))


def kappa(l, dH, L):
    """First-order amplification of one rounding of the inputs into u (0 where there is no root):
    du/u = r / (cosh u - r) dr/r from sinh u = r u, and dr/r from (l, dH, L) through r = sqrt(L^2 - dH^2) / l."""
    l, dH, L = float(l), float(dH), float(L)
    if true_root(l, dH, L) is None:
        return 0.0
    u, _, r = _root_cached(l, dH, L)
    with mp.workdps(DPS):
        return float(_kappa_mp(u, r, mpf(dH), mpf(L)))


def tension_true(l, dH, L, w_per_len, c_lo, c_hi):
    """w l / (2 sinh u*) as mpf; the fallback w l / 2 where there is no root in [c_lo, c_hi] (a float where l is not finite)."""
    l, w = float(l), float(w_per_len)
    root = true_root(l, dH, L)
    if not (math.isfinite(l) and math.isfinite(w)):
        return w * l / 2
    with mp.workdps(DPS):
        if root is None or not (c_lo <= root[1] <= c_hi):
            return mpf(w) * mpf(l) / 2
        return mpf(w) * mpf(l) / (2 * mp.sinh(root[0]))


# ---- lowest point of the augmented shape ----------------------------------------------------------------------------

def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return mp.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _rod(v, axis, ang):
    n = _norm(axis)
    k = [a / n for a in axis]
    c, s = mp.cos(ang), mp.sin(ang)
    kv = _cross(k, v)
    kd = (k[0] * v[0] + k[1] * v[1] + k[2] * v[2]) * (1 - c)
    return [v[i] * c + kv[i] * s + k[i] * kd for i in range(3)]


def _axes(rel):
    xy = [rel[0], rel[1], mpf(0)]
    nxy = _norm(xy)
    xy = [mpf(1), mpf(0), mpf(0)] if nxy < mpf("1e-9") else [x / nxy for x in xy]
    th = _cross(xy, [mpf(0), mpf(0), mpf(1)])
    nth = _norm(th)
    th = [mpf(0), mpf(1), mpf(0)] if nth < mpf("1e-9") else [x / nth for x in th]
    nr = _norm(rel)
    return th, [x / nr for x in rel]


LowZ = collections.namedtuple("LowZ", "z valid u kappa lp dHp r u_cold")


def lowest_z_true(P0, P, th, ga, L, M, up, c_lo, c_hi):
    """oracle.augmented_lowest_z_vec for one point at 50 digits: axes, theta-rotated end point and its catenary, M samples
    turned back by -theta and by +gamma, the minimum in the "up" sense; the straight segment [A, B'] where the rotated
    end point has no root in the bracket.  Also returns that solve's u', kappa', (l', dH', r') and the cold solve's u."""
    with mp.workdps(DPS):
        P0 = [_mp(x) for x in P0]; P = [_mp(x) for x in P]
        th, ga, L, up = _mp(th), _mp(ga), _mp(L), _mp(up)
        rel = [P[i] - P0[i] for i in range(3)]
        cold = _root_mp(mp.sqrt(rel[0] ** 2 + rel[1] ** 2), up * rel[2], L)
        th_axis, ga_axis = _axes(rel)
        Bp = _rod(rel, th_axis, th)
        lp = mp.sqrt(Bp[0] ** 2 + Bp[1] ** 2)
        dHp = up * Bp[2]
        root = _root_mp(lp, dHp, L)
        valid = root is not None and c_lo <= root[1] <= c_hi
        if valid:
            u, C, r = root
            x0 = lp / 2 - mp.atanh(dHp / L) / C
            ch0 = mp.cosh(C * x0)
            best = mp.inf
            for j in range(M):
                t = mpf(j) / (M - 1)
                up_j = (mp.cosh(C * (lp * t - x0)) - ch0) / C
                q = [t * Bp[0], t * Bp[1], up * up_j]
                q = _rod(q, th_axis, -th)
                q = _rod(q, ga_axis, ga)
                best = min(best, up * (P0[2] + q[2]))
            kap = float(_kappa_mp(u, r, dHp, L))
        else:
            qb = _rod(_rod(Bp, th_axis, -th), ga_axis, ga)
            best = min(up * P0[2], up * (P0[2] + qb[2]))
            u, r, kap = (root[0], root[2], float(_kappa_mp(root[0], root[2], dHp, L))) if root is not None else (None, None, 0.0)
        return LowZ(up * best, valid, None if u is None else float(u), kap if valid else 0.0, float(lp), float(dHp),
                    None if r is None else float(r), None if cold is None else float(cold[0]))


# ---- the point set ------------------------------------------------------------------------------------------------------

def _dH_for(r, l, L, sign):
    """dH = sign * sqrt(L^2 - r^2 l^2) rounded to double, or None when r l > L (such a combination is not generated)."""
    with mp.workdps(DPS):
        s = mpf(L) ** 2 - (r * mpf(l)) ** 2
        if s < 0:
            return None
        return sign * float(mp.sqrt(s))


def _r_of_u(u):
    return mp.sinh(u) / u


@functools.lru_cache(maxsize=None)
def workspace(L=L_WS):
    """The deterministic point set, about 330 points.  Each point is built from a target u: r = sinh(u) / u and
    dH = +-sqrt(L^2 - r^2 l^2) rounded to double (a target with r l > L is not generated: with l >= 0.05 that ends family (a)
    near u = 5.6); the root is then recomputed from the rounded doubles."""
    pts = []
    with mp.workdps(DPS):
        def add(family, tag, l, r, sign):
            dH = _dH_for(r, l, L, sign)
            if dH is not None:
                pts.append(Point(family, tag, float(l), dH, float(L)))

        # (a) u log-spaced from 1e-4 to 14, 40 values per l, dH alternating in sign
        us = [mpf(10) ** (mp.log10(mpf("1e-4")) + (mp.log10(14) - mp.log10(mpf("1e-4"))) * i / 39) for i in range(40)]
        for l in LS:
            for i, u in enumerate(us):
                add("a", "u=%.3g" % float(u), l, _r_of_u(u), 1 if i % 2 == 0 else -1)
        # (b) the series switch u = 0.5 and the logarithmic start r = 8, approached from both sides
        for l in LS:
            for k in (10, 20, 30, 40):
                for sgn in (1, -1):
                    u = mpf("0.5") * (1 + sgn * mpf(2) ** -k)
                    add("b", "u=0.5(1%+d*2^-%d)" % (sgn, k), l, _r_of_u(u), sgn)
                    add("b", "r=8(1%+d*2^-%d)" % (sgn, k), l, 8 * (1 + sgn * mpf(2) ** -k), -sgn)
        # (c) C* at the ends of the narrow bracket
        for c_end, name, ls in ((C_NARROW[1], "c_hi", (0.3, 1.0)), (C_NARROW[0], "c_lo", (1.0, 2.5))):
            for l in ls:
                for delta in ("1e-3", "1e-6", "1e-9"):
                    for sgn in (1, -1):
                        u = mpf(c_end) * (1 + sgn * mpf(delta)) * mpf(l) / 2
                        add("c", "%s(1%+d*%s)" % (name, sgn, delta), l, _r_of_u(u), 1)
        # (d) L - |dH| = 2^-k L with a small valid l (l = sqrt(L^2 - dH^2) / r for a chosen u)
        for k in (10, 30, 50):
            for sgn in (1, -1):
                dH = sgn * (L - 2.0 ** -k * L)
                for u in ("2", "5"):
                    l = float(mp.sqrt(mpf(L) ** 2 - mpf(dH) ** 2) / _r_of_u(mpf(u)))
                    pts.append(Point("d", "k=%d,u=%s" % (k, u), l, dH, float(L)))
    # (e) no root
    nan, inf = math.nan, math.inf
    pts += [Point("e", "taut exactly", 3.0, 4.0, 5.0), Point("e", "beyond taut", 2.5, 2.0, L), Point("e", "beyond taut", 2.99, -1.0, L),
            Point("e", "l=0", 0.0, 1.0, L), Point("e", "l=0", 0.0, 0.0, L), Point("e", "|dH|=L", 0.3, L, L), Point("e", "|dH|=L", 0.3, -L, L),
            Point("e", "|dH|>L", 0.3, 3.5, L), Point("e", "|dH|>L", 0.3, -4.0, L)]
    for bad in (nan, inf, -inf):
        pts += [Point("e", "l=%r" % bad, bad, 1.0, L), Point("e", "dH=%r" % bad, 1.0, bad, L), Point("e", "L=%r" % bad, 1.0, 1.0, bad)]
    return tuple(pts)


# ---- bounds -------------------------------------------------------------------------------------------------------------

Table = collections.namedtuple("Table", "pts C u kap E_ref scale_C T_root T_fb E_T_ref scale_T xtol_T C_mp T_mp")


@functools.lru_cache(maxsize=None)
def table(L=L_WS, w_wet=W_WET):
    """Per point: C*, u*, kappa (NaN / 0 where there is no root), the plain fp64 reference's errors E_ref (brentq, with a
    bracket that holds the root and keeps f finite) and E_T_ref, and the conditioning scales eps (1 + kappa) |C*| and
    eps (1 + kappa_T) |T*|, kappa_T = kappa u coth u (dT/T = -u coth u du/u)."""
    from oracle import rovmpc_oracle as orc
    pts = workspace(L)
    n = len(pts)
    C = np.full(n, np.nan); u = np.full(n, np.nan); kap = np.zeros(n); E = np.zeros(n); sC = np.zeros(n)
    Tr = np.full(n, np.nan); Tf = np.zeros(n); ET = np.zeros(n); sT = np.zeros(n); xT = np.zeros(n)
    Cm = [None] * n; Tmp = [None] * n
    for i, p in enumerate(pts):
        with np.errstate(all="ignore"):
            w = w_wet / p.L
            Tf[i] = w * p.l / 2
        root = true_root(p.l, p.dH, p.L)
        if root is None:
            continue
        us, Cs = root
        with mp.workdps(DPS):
            Tm = mpf(w) * mpf(p.l) / (2 * mp.sinh(us))
            ucoth = float(us / mp.tanh(us))
        Cm[i], Tmp[i] = Cs, Tm
        C[i], u[i], kap[i], Tr[i] = float(Cs), float(us), kappa(p.l, p.dH, p.L), float(Tm)
        sC[i] = EPS * (1 + kap[i]) * abs(C[i])
        sT[i] = EPS * (1 + kap[i] * ucoth) * abs(Tr[i])
        xT[i] = XTOL * Tr[i] * ucoth / C[i]                        # |dT/dC| * xtol, dT/dC = -T coth(u) l / 2 = -T u coth(u) / C
        c_ref = float(orc.solve_catenary_ref(p.l, p.dH, p.L, C_WIDE[0], min(C_WIDE[1], 1400.0 / p.l)))
        if math.isfinite(c_ref):
            E[i] = abs(float(mpf(c_ref) - Cs))
            ET[i] = abs(float(mpf(float(orc.cable_tension(p.l, c_ref, p.L, w_wet))) - Tm))
        else:
            E[i] = ET[i] = np.nan                                   # the plain reference finds no root where there is one
    return Table(pts, C, u, kap, E, sC, Tr, Tf, ET, sT, xT, Cm, Tmp)


def measured_margins(L=L_WS):
    """(ratio_C, ratio_T): the largest E_ref_i / (eps (1 + kappa_i) |C*_i| + xtol) over the valid points, and the same for the tension."""
    t = table(L)
    ok = np.isfinite(t.C) & np.isfinite(t.E_ref)
    return float(np.max(t.E_ref[ok] / (t.scale_C[ok] + XTOL))), float(np.max(t.E_T_ref[ok] / (t.scale_T[ok] + t.xtol_T[ok])))


def bounds(L=L_WS):
    """(bound_C, bound_T) per point: m * max(E_ref_i, scale_i); 0 where there is no root (the fallback tension has its own)."""
    t = table(L)
    E = np.where(np.isfinite(t.E_ref), t.E_ref, 0.0); ET = np.where(np.isfinite(t.E_T_ref), t.E_T_ref, 0.0)
    return M_C * np.maximum(E, t.scale_C), M_T * np.maximum(ET, t.scale_T)


def validity(c_lo, c_hi, L=L_WS):
    """(valid, undecided): C* inside [c_lo, c_hi]; undecided where C* is within bound_i of a bracket end (either answer is acceptable)."""
    t = table(L)
    bC, _ = bounds(L)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(t.C) & (t.C >= c_lo) & (t.C <= c_hi)
        und = np.isfinite(t.C) & ((np.abs(t.C - c_lo) <= bC) | (np.abs(t.C - c_hi) <= bC))
    return valid, [int(i) for i in np.nonzero(und)[0]]


def expected_tension(c_lo, c_hi, L=L_WS):
    """(T*, bound) per point on an engine with bracket [c_lo, c_hi]: the root's tension where C* is valid, else w l / 2
    (two roundings: bound m * eps |T|; exact where it is 0 or not finite)."""
    t = table(L)
    valid, _ = validity(c_lo, c_hi, L)
    _, bT = bounds(L)
    with np.errstate(invalid="ignore"):
        fb_bound = np.where(np.isfinite(t.T_fb), M_T * EPS * np.abs(t.T_fb), 0.0)
    return np.where(valid, t.T_root, t.T_fb), np.where(valid, bT, fb_bound)


# ---- lowest-point cases ---------------------------------------------------------------------------------------------

ANGLES = (0.0, 0.05, -0.05, 0.6, -0.6)
MS = (2, 3, 4, 16, 17)


@functools.lru_cache(maxsize=None)
def shape_geometry(L=L_WS):
    """24 connection vectors (rel, ENU sense: z up) for the lowest-point checks: near-taut ones (u' < 0.5 after the rotation,
    and a warm start that the rotation invalidates), slack ones, steep ones, a vertical one and three beyond taut (straight-segment fallback)."""
    g = []
    for i, (d_over_L, elev) in enumerate(((0.999, 0.3), (0.995, -0.8), (0.98, 1.1), (0.97, -0.2), (0.95, 0.6), (0.9, -1.2),
                                          (0.8, 0.1), (0.7, -0.5), (0.6, 1.3), (0.5, -0.9), (0.35, 0.4), (0.2, -0.3),
                                          (0.1, 0.7), (0.05, -1.0), (0.9, 0.0), (0.999, -1.3), (0.99, 0.02), (0.3, 1.45),
                                          (0.6, -1.5), (0.85, 0.75))):
        d = d_over_L * L
        phi = 0.7 * i + 0.1
        g.append((d * math.cos(elev) * math.cos(phi), d * math.cos(elev) * math.sin(phi), d * math.sin(elev)))
    g.append((0.0, 0.0, -1.4))                                        # vertical: degenerate xy projection
    g += [(2.9, 1.2, 0.4), (0.5, -0.4, 3.2), (1.05 * L, 0.0, 0.0)]     # beyond taut
    return tuple(g)


def shape_cases(L=L_WS):
    """At most 120 (rel, theta, gamma, M, up) for the stand-alone lowest-point check: every geometry with five (theta, gamma, M)."""
    out = []
    for i, rel in enumerate(shape_geometry(L)):
        for j in range(5):
            out.append((rel, ANGLES[(i + 2 * j) % 5], ANGLES[(3 * i + j + 1) % 5], MS[(i + j) % 5], 1.0 if (i + j) % 2 == 0 else -1.0))
    return out


def z_scale(kap, L=L_WS, eps=EPS):
    return eps * L * (1 + kap)
