"""The cable chain of csrc/device_math.h against the 50-digit reference of tests/cable_reference.py: the catenary root,
the tension and the lowest point of the augmented shape, through the stand-alone entry points (fp64, cold start) and through
the rollout's own instantiations (warm start, fp32, augmented_finish at several M, the three model paths).

Bounds are per point: m * max(E_ref_i, eps (1 + kappa_i) |x*_i|) with the margins m that test_cable_reference_host.py
measures on the plain fp64 reference.  Each test prints its largest ratio against the bound before it asserts."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import cable_reference as cr

pytestmark = pytest.mark.gpu

EPS, EPS32 = cr.EPS, cr.EPS32
L = cr.L_WS


@pytest.fixture(scope="module")
def rv():
    import rovmpc
    return rovmpc


def _same_L(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _solve_all(rv, bracket, pts):
    """(C, T) of every point through the stand-alone entry points: one call per distinct L (L is a scalar argument)."""
    C = np.empty(len(pts)); T = np.empty(len(pts))
    done = np.zeros(len(pts), bool)
    for p in pts:
        idx = [i for i, q in enumerate(pts) if not done[i] and _same_L(q.L, p.L)]
        if not idx:
            continue
        l = np.array([pts[i].l for i in idx]); dH = np.array([pts[i].dH for i in idx])
        if bracket == cr.C_DEFAULT:
            c = rv.solve_catenary(l, dH, p.L)
            c2, t = rv.cable_tension(l, dH, p.L, cr.W_WET)
            assert np.array_equal(c, c2, equal_nan=True)
        else:
            c, t = rv.Catenary(L, "ENU", 2, *bracket)._engine().solve_catenary(l, dH, p.L, with_tension=True)
        C[idx] = c; T[idx] = t; done[idx] = True
    return C, T


def _mp_err(x, ref):
    with mp.workdps(cr.DPS):
        return float(abs(mpf(float(x)) - ref))


@pytest.mark.parametrize("bracket", [cr.C_DEFAULT, cr.C_NARROW, cr.C_WIDE], ids=["default", "narrow", "wide"])
def test_root_and_tension_at_every_workspace_point(rv, bracket):
    t = cr.table()
    bC, bT = cr.bounds()
    valid, und = cr.validity(*bracket)
    Texp, bTexp = cr.expected_tension(*bracket)
    C, T = _solve_all(rv, bracket, t.pts)
    worst_C = worst_T = 0.0
    bad = []
    with mp.workdps(cr.DPS):
        for i, p in enumerate(t.pts):
            if i in und:                                            # either answer, but one of the two
                ok = math.isnan(C[i]) or _mp_err(C[i], t.C_mp[i]) <= bC[i]
                okT = _mp_err(T[i], t.T_mp[i]) <= bT[i] or abs(T[i] - t.T_fb[i]) <= cr.M_T * EPS * abs(t.T_fb[i])
                if not (ok and okT):
                    bad.append((p, C[i], T[i]))
                continue
            if math.isnan(C[i]) != (not valid[i]):
                bad.append((p, "C", C[i], t.C[i])); continue
            if valid[i]:
                e = _mp_err(C[i], t.C_mp[i]); worst_C = max(worst_C, e / bC[i] * cr.M_C)
                eT = _mp_err(T[i], t.T_mp[i]); worst_T = max(worst_T, eT / bT[i] * cr.M_T)
                if e > bC[i] or eT > bT[i]:
                    bad.append((p, "err", e / bC[i] * cr.M_C, eT / bT[i] * cr.M_T))
            elif math.isfinite(Texp[i]):
                eT = abs(T[i] - Texp[i])
                if bTexp[i] > 0:
                    worst_T = max(worst_T, eT / bTexp[i] * cr.M_T)
                if not eT <= bTexp[i]:
                    bad.append((p, "fallback", T[i], Texp[i]))
            elif not ((math.isnan(T[i]) and math.isnan(Texp[i])) or T[i] == Texp[i]):
                bad.append((p, "fallback", T[i], Texp[i]))
    print("bracket %s: largest ratio C %.3f of m = %g, tension %.3f of m = %g, undecided %s"
          % (bracket, worst_C, cr.M_C, worst_T, cr.M_T, [t.pts[i] for i in und]))
    assert not bad, bad


def test_results_do_not_depend_on_the_position_in_the_launch(rv):
    """The L = 3 points as one call, as 257 and 513 entries (cyclic padding / prefix) and shifted by one entry: the 256-thread
    kernel's block edges fall elsewhere each time, and every point's (C, T) is bit-equal."""
    pts = [p for p in cr.workspace() if p.L == L]
    l = np.array([p.l for p in pts]); dH = np.array([p.dH for p in pts])
    eng = rv.Catenary(L, "ENU", 2, *cr.C_WIDE)._engine()
    C0, T0 = eng.solve_catenary(l, dH, L, with_tension=True)
    for n, shift in ((257, 0), (513, 0), (len(pts) + 1, 1), (513, 255)):
        idx = (np.arange(n) - shift) % len(pts)
        C, T = eng.solve_catenary(l[idx], dH[idx], L, with_tension=True)
        assert np.array_equal(C, C0[idx], equal_nan=True) and np.array_equal(T, T0[idx], equal_nan=True), (n, shift)


@pytest.mark.parametrize("M,frame", [(2, "ENU"), (3, "NED"), (16, "ENU")])
def test_catenary_points_against_50_digits(rv, M, frame):
    """First and last sample are A and B (the last one's sag term, which is dH, within the C-scaled tolerance of a sample), params are
    (C, (cosh(C x0) - 1) / C, x0) and every interior sample lies on z = (cosh(C (x - x0)) - cosh(C x0)) / C, all against
    50-digit values.  Tolerance of a quantity q(C, a), a = atanh(dH / L): |dq/dC| bound_C + |dq/da| da + its own roundings,
    da = 2 eps (|q| / (1 - q^2) + |a|) with q = dH / L (one rounding of the quotient through atanh', and atanh's own),
    roundings 4 eps (1 + |arg| + 2u) cosh(arg) / C per cosh."""
    t = cr.table()
    bC, _ = cr.bounds()
    up = 1.0 if frame == "ENU" else -1.0
    idx = [i for i, p in enumerate(t.pts) if p.L == L and np.isfinite(t.C[i])][::3]
    B = np.array([[t.pts[i].l, 0.0, up * t.pts[i].dH] for i in idx])
    pts, valid, params = rv.Catenary(L, frame, M, *cr.C_WIDE).batch(np.zeros_like(B), B)
    assert valid.all()
    worst = 0.0
    bad = []
    with mp.workdps(cr.DPS):
        for k, i in enumerate(idx):
            p = t.pts[i]
            l, dH, C, u = mpf(p.l), mpf(p.dH), t.C_mp[i], mpf(t.u[i])
            q = dH / mpf(L)
            a = mp.atanh(q)
            x0 = l / 2 - a / C
            relC = mpf(bC[i]) / C
            da = 2 * EPS * (abs(q) / (1 - q * q) + abs(a))
            arg2 = C * x0
            sh2, ch2 = abs(mp.sinh(arg2)), mp.cosh(arg2)
            assert np.array_equal(pts[k, 0], [0.0, 0.0, 0.0]) and pts[k, M - 1, 0] == p.l and pts[k, M - 1, 1] == 0.0
            checks = [("C", params[k, 0], C, mpf(bC[i])),
                      ("x0", params[k, 2], x0, abs(a / C) * relC + da / C + 4 * EPS * (l / 2 + abs(a / C))),
                      ("sag", params[k, 1], (ch2 - 1) / C,
                       relC * (l / 2 * sh2 + (ch2 - 1) / C) + da * sh2 / C + 4 * EPS * (1 + abs(arg2) + 2 * u) * ch2 / C)]
            for j in range(1, M):
                tj = mpf(j) / (M - 1)
                arg1 = C * (l * tj - x0)
                sh1, ch1 = abs(mp.sinh(arg1)), mp.cosh(arg1)
                z = (ch1 - ch2) / C
                tol = (relC * (abs(l * tj - l / 2) * sh1 + l / 2 * sh2 + abs(z)) + da * (sh1 + sh2) / C
                       + 4 * EPS * (1 + abs(arg1) + abs(arg2) + 2 * u) * (ch1 + ch2) / C)
                checks.append(("z%d" % j, up * pts[k, j, 2], z, tol))
                if j < M - 1:
                    assert abs(pts[k, j, 0] - float(l * tj)) <= 2 * EPS * p.l and pts[k, j, 1] == 0.0
            for name, got, ref, tol in checks:
                e = abs(mpf(float(got)) - ref)
                worst = max(worst, float(e / tol))
                if not e <= tol:
                    bad.append((p, name, float(got), float(ref), float(e / tol)))
    print("catenary_points M = %d %s: largest error / tolerance %.3f over %d points" % (M, frame, worst, len(idx)))
    assert not bad, bad[:10]


@pytest.fixture(scope="module")
def shape_truth():
    return [cr.lowest_z_true((0.0, 0.0, 0.0), (rel[0], rel[1], up * rel[2]), th, ga, L, M, up, *cr.C_SHAPE)
            for rel, th, ga, M, up in cr.shape_cases()]


def test_transform_catenary_batch_lowest_point(rv, shape_truth):
    cases = cr.shape_cases()
    worst = 0.0
    bad = []
    for M in cr.MS:
        for up in (1.0, -1.0):
            idx = [i for i, c in enumerate(cases) if c[3] == M and c[4] == up]
            if not idx:
                continue
            B = np.array([[cases[i][0][0], cases[i][0][1], up * cases[i][0][2]] for i in idx])
            cat = rv.Catenary(L, "ENU" if up > 0 else "NED", M, *cr.C_SHAPE)
            _, npts, z = rv.transform_catenary_batch(np.zeros_like(B), B, np.array([cases[i][1] for i in idx]),
                                                     np.array([cases[i][2] for i in idx]), cat)
            for k, i in enumerate(idx):
                tr = shape_truth[i]
                assert (npts[k, 1] == M) == tr.valid or M == 2, cases[i]
                ratio = _mp_err(z[k], tr.z) / cr.z_scale(tr.kappa)
                worst = max(worst, ratio)
                if not ratio <= cr.M_Z:
                    bad.append((cases[i], float(z[k]), float(tr.z), ratio))
    print("transform_catenary_batch: largest ratio %.3f of m_z = %g" % (worst, cr.M_Z))
    assert not bad, bad


# ---- the rollout's own instantiations -----------------------------------------------------------------------------------

DT = 1.0 / 64          # with v_scale = 1 and P0 = P1 = 0 the node is P = U / 64 exactly, in fp64 and in fp32


class Rollouts:
    """Engines with N = 1, vt_mode = 0 and every weight zero but those named; candidate k of a launch lands on rel[k]."""

    def __init__(self, rv):
        self.rv, self.engines = rv, {}

    def engine(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self.engines:
            cfg = dict(N=1, vt_mode=0, dt=DT, v_scale=1.0, L=L, cable_wet_weight=cr.W_WET, w_theta=0.0, w_gamma=0.0, w_u=0.0,
                       w_T=0.0, w_taut=0.0, w_floor=0.0)
            cfg.update(kw)
            self.engines[key] = self.rv.Engine(self.rv.MPCConfig(**cfg))
        return self.engines[key]

    def run(self, rels, theta=0.0, gamma=0.0, **kw):
        """(J (n,), (theta, gamma) at node 1 (n, 2)) for n connection vectors, K per launch, the last launch padded cyclically."""
        e = self.engine(**kw)
        K = kw["K"]
        rels = np.asarray(rels, np.float64)
        n = len(rels)
        state = np.zeros(16); state[12:16] = (theta, gamma, theta, gamma)
        J = np.empty(n, e.cfg.np_dtype); tr = np.empty((n, 2), e.cfg.np_dtype)
        for s in range(0, n, K):
            idx = np.arange(s, s + K) % n
            Jc, tc = e.rollout_costs(state, (rels[idx] * 64.0).reshape(K, 1, 3), return_traj=True)
            m = min(K, n - s)
            J[s:s + m] = Jc[:m]; tr[s:s + m] = tc[:m, 1]
        return J, tr

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def ro(rv):
    r = Rollouts(rv)
    yield r
    r.close()


def _rollout_points():
    """Workspace points a rollout can be put on: the engine's own L, finite coordinates (a non-finite control is a NaN cost,
    which test_nan_costs_never_win covers)."""
    t = cr.table()
    return [i for i, p in enumerate(t.pts) if p.L == L and math.isfinite(p.l) and math.isfinite(p.dH)]


def _tension_case(dtype, bracket):
    """(rels, T*, bound, used) per rollout point: fp64 from the table; fp32 from the fp32-rounded coordinates and w / L, on the
    eps32 scale, only where eps32 * kappa < 1e-3 (and, without a root, only family (e))."""
    t = cr.table()
    idx = _rollout_points()
    rels = np.array([[t.pts[i].l, 0.0, t.pts[i].dH] for i in idx])
    if dtype == "f64":
        Texp, b = cr.expected_tension(*bracket)
        valid, und = cr.validity(*bracket)
        return rels, [t.T_mp[i] if valid[i] else mpf(t.T_fb[i]) for i in idx], b[idx], np.array([i not in und for i in idx])
    rels = rels.astype(np.float32).astype(np.float64)
    w = float(np.float32(cr.W_WET / L))
    T, b, used = [], [], []
    for k, i in enumerate(idx):
        l, dH = rels[k, 0], rels[k, 2]
        root = cr.true_root(l, dH, L)
        kap = cr.kappa(l, dH, L)
        Tm = cr.tension_true(l, dH, L, w, *bracket)
        T.append(Tm)
        if root is None or not (bracket[0] <= root[1] <= bracket[1]):
            used.append(root is None and t.pts[i].family == "e")
            b.append(cr.M_T * EPS32 * abs(float(Tm)))
        else:
            used.append(EPS32 * kap < 1e-3 and min(abs(float(root[1]) / bracket[0] - 1), abs(float(root[1]) / bracket[1] - 1)) > 1e-3)
            with mp.workdps(cr.DPS):
                b.append(cr.M_T * EPS32 * (1 + kap * float(root[0] / mp.tanh(root[0]))) * abs(float(Tm)))
    return rels, T, np.array(b), np.array(used)


def _check_tension(J, T, b, used, label):
    worst, bad = 0.0, []
    for k in range(len(J)):
        if not used[k]:
            continue
        e = _mp_err(J[k], T[k])
        if b[k] > 0:
            worst = max(worst, e / b[k] * cr.M_T)
        if not e <= b[k]:
            bad.append((k, float(J[k]), float(T[k]), e, b[k]))
    print("%s: largest ratio %.3f of m = %g over %d points" % (label, worst, cr.M_T, int(np.sum(used))))
    assert not bad, bad[:10]


@pytest.mark.parametrize("K", [64, 67])
@pytest.mark.parametrize("dtype,bracket", [("f64", cr.C_WIDE), ("f64", cr.C_NARROW), ("f32", cr.C_WIDE)],
                         ids=["f64-wide", "f64-narrow", "f32-wide"])
def test_rollout_tension_term(ro, dtype, bracket, K):
    """w_T = 1 alone: J[k] is the tension of the cold solve_catenary_root<T> of phase 4a."""
    rels, T, b, used = _tension_case(dtype, bracket)
    J, _ = ro.run(rels, K=K, dtype=dtype, w_T=1.0, c_lo=bracket[0], c_hi=bracket[1])
    assert ro.engine(K=K, dtype=dtype, w_T=1.0, c_lo=bracket[0], c_hi=bracket[1]).model_path == "builtin"
    assert used.sum() > (150 if dtype == "f64" else 60)
    _check_tension(J, T, b, used, "rollout tension %s K = %d bracket %s" % (dtype, K, bracket))


@pytest.mark.parametrize("K", [64, 67])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rollout_taut_term(ro, dtype, K):
    """w_taut = 1 alone, rho_taut = 0.9: J = max(0, d - 0.9 L)^2.  No solve in it: it guards the plane indexing the other terms
    rely on.  The 4 ulp are those of d = |rel|, where the roundings are: d - 0.9 L cancels, so J itself carries
    2 d / (d - 0.9 L) times the relative error of d and no fixed number of its own ulps can hold."""
    t = cr.table()
    eps = EPS if dtype == "f64" else EPS32
    rels = np.array([[t.pts[i].l, 0.0, t.pts[i].dH] for i in _rollout_points()])
    if dtype == "f32":
        rels = rels.astype(np.float32).astype(np.float64)
    J, _ = ro.run(rels, K=K, dtype=dtype, w_taut=1.0, rho_taut=0.9)
    rhoL = 0.9 * L if dtype == "f64" else float(np.float32(0.9 * L))
    worst, bad, pos = 0.0, [], 0
    with mp.workdps(cr.DPS):
        for k, r in enumerate(rels):
            d = mp.sqrt(mpf(r[0]) ** 2 + mpf(r[2]) ** 2)
            tol = 4 * eps * d
            if d < rhoL - tol:
                ok = J[k] == 0
            else:
                e = abs(mp.sqrt(mpf(float(J[k]))) - max(d - rhoL, 0))
                worst = max(worst, float(e / tol)); ok = e <= tol; pos += 1
            if not ok:
                bad.append((tuple(r), float(J[k]), float(d - rhoL)))
    print("rollout taut term %s K = %d: largest error %.3f of 4 ulp of d, %d points beyond 0.9 L" % (dtype, K, worst, pos))
    assert pos > 50 and not bad, bad[:10]


ANGLE_PAIRS_BIG = ((0.6, -0.05), (-0.6, 0.05), (0.6, 0.6))
ANGLE_PAIRS_SMALL = ((0.05, -0.6), (0.0, 0.0), (-0.05, 0.6))


def _floor_check(ro, dtype, frame, M, K, pairs, label, **kw):
    """w_floor = 1 alone, z_floor one metre above the anchor in the "up" sense: z_low = z_floor - up sqrt(J) is the lowest point
    from the warm-started solve and augmented_finish.  Returns J per angle pair."""
    up = 1.0 if frame == "ENU" else -1.0
    eps = EPS if dtype == "f64" else EPS32
    rels = np.array([[g[0], g[1], up * g[2]] for g in cr.shape_geometry()])
    if dtype == "f32":
        rels = rels.astype(np.float32).astype(np.float64)
    z_floor = up * 1.0
    worst, bad, out = 0.0, [], []
    n_none = n_rejected = n_series = n_used = 0
    for th0, ga0 in pairs:
        J, tr = ro.run(rels, theta=th0, gamma=ga0, K=K, dtype=dtype, frame=frame, n_shape_pts=M, w_floor=1.0, z_floor=z_floor,
                       c_lo=cr.C_SHAPE[0], c_hi=cr.C_SHAPE[1], **kw)
        out.append(J)
        for k, r in enumerate(rels):
            t = cr.lowest_z_true((0.0, 0.0, 0.0), r, float(tr[k, 0]), float(tr[k, 1]), L, M, up, *cr.C_SHAPE)
            d = math.sqrt(r[0] ** 2 + r[1] ** 2 + r[2] ** 2)
            if t.valid:
                C = 2 * t.u / t.lp
                used = dtype == "f64" or (EPS32 * t.kappa < 1e-3 and min(abs(C / cr.C_SHAPE[0] - 1), abs(C / cr.C_SHAPE[1] - 1)) > 1e-3)
            else:                                  # fp32: only where its own roundings cannot bring the root back
                used = dtype == "f64" or (d > L * (1 + 1e-3) if t.u is None else abs(2 * t.u / t.lp / cr.C_SHAPE[1] - 1) > 1e-3)
            if not used:
                continue
            n_used += 1
            n_none += not t.valid
            n_rejected += bool(t.valid and t.u_cold is not None and t.r >= math.cosh(t.u_cold))
            n_series += bool(t.valid and t.u < 0.5)
            z = z_floor - up * math.sqrt(float(J[k]))
            tol = cr.M_Z * cr.z_scale(t.kappa, L, eps) + eps * abs(z_floor)
            e = _mp_err(z, t.z)
            worst = max(worst, e / tol * cr.M_Z)
            if not e <= tol:
                bad.append((tuple(r), th0, ga0, z, float(t.z), e / tol * cr.M_Z, t.valid, t.u, t.kappa))
    print("%s: largest ratio %.3f of m_z = %g over %d points (%d without a root, %d with the warm start rejected, %d with u' < 0.5)"
          % (label, worst, cr.M_Z, n_used, n_none, n_rejected, n_series))
    assert n_none >= 1 and n_rejected >= 1 and n_series >= 1
    assert not bad, bad[:10]
    return out


@pytest.mark.parametrize("M", cr.MS)
@pytest.mark.parametrize("frame", ["ENU", "NED"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rollout_floor_term(ro, dtype, frame, M):
    i = cr.MS.index(M) + (frame == "NED")
    pairs = (ANGLE_PAIRS_BIG[i % 3], ANGLE_PAIRS_SMALL[(i + 1) % 3])
    for K in (64, 67):
        _floor_check(ro, dtype, frame, M, K, pairs, "rollout floor term %s %s M = %d K = %d" % (dtype, frame, M, K))


PATHS = (("interpreter", dict(force_interpreter=True)), ("jit", dict(no_builtin=True)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_model_paths_share_the_geometry(ro, dtype):
    """The interpreter and the hiprtc-specialised kernel of the same rows: tension and floor term within the same bounds as
    the compiled-in kernel.  The floor term reads (theta, gamma) of node 1, which each path integrates with its own
    arithmetic, and sincos(gamma) from a source of its own (gamma table of the compiled-in kernel, table of the
    specialised one, a call in the interpreter): no two paths share it, so there each is held to the bound alone."""
    rels, T, b, used = _tension_case(dtype, cr.C_WIDE)
    kwT = dict(K=64, dtype=dtype, w_T=1.0, c_lo=cr.C_WIDE[0], c_hi=cr.C_WIDE[1])
    for path, kw in PATHS:
        J, _ = ro.run(rels, **kwT, **kw)
        assert ro.engine(**kwT, **kw).model_path == path
        _check_tension(J, T, b, used, "rollout tension %s %s" % (dtype, path))
        _floor_check(ro, dtype, "ENU", 16, 64, (ANGLE_PAIRS_BIG[0], ANGLE_PAIRS_SMALL[0]), "rollout floor term %s %s M = 16" % (dtype, path), **kw)


@pytest.mark.parametrize("path,kw", PATHS, ids=[p for p, _ in PATHS])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_model_paths_tension_bit_equal(ro, dtype, path, kw):
    """The tension term reads neither angle, so no sincos source is involved: every path must give the compiled-in kernel's bits.

    (Before the cable chain of device_math.h fixed its contraction mode, the hiprtc build of the fp32 chain rounded one
    expression differently and the family (b) point l = 0.05 next to u = 0.5 took the other branch there: 6e-7 relative.)"""
    rels, _, _, _ = _tension_case(dtype, cr.C_WIDE)
    kwT = dict(K=64, dtype=dtype, w_T=1.0, c_lo=cr.C_WIDE[0], c_hi=cr.C_WIDE[1])
    J0, _ = ro.run(rels, **kwT)
    J, _ = ro.run(rels, **kwT, **kw)
    diff = np.nonzero(~((J == J0) | (np.isnan(J) & np.isnan(J0))))[0]
    with np.errstate(all="ignore"):
        print("tension %s %s against builtin: %d of %d points differ, largest |dJ| / J = %.3g"
              % (dtype, path, len(diff), len(J), float(np.max(np.abs(J[diff] - J0[diff]) / np.abs(J0[diff]))) if len(diff) else 0.0))
    assert len(diff) == 0, [(tuple(rels[k]), float(J[k]), float(J0[k])) for k in diff[:10]]
