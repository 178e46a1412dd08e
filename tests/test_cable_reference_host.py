"""CPU check of the 50-digit cable reference and of the bounds the GPU tests use (tests/cable_reference.py): the root's
residual, the margins measured on the plain fp64 reference (brentq / the oracle's lowest point), and the validity rule."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import cable_reference as cr


@pytest.fixture(scope="module")
def orc():
    from oracle import rovmpc_oracle
    return rovmpc_oracle


def test_workspace_families():
    pts = cr.workspace()
    fam = {f: [p for p in pts if p.family == f] for f in "abcde"}
    assert len(pts) <= 1500 and all(len(v) > 0 for v in fam.values())
    assert pts == cr.workspace()                                    # deterministic
    t = cr.table()
    # every generated point of (a)-(d) has a root, no point of (e) has one
    for i, p in enumerate(pts):
        assert np.isfinite(t.C[i]) == (p.family != "e"), p
    # the construction reaches what it is for: both sides of u = 0.5 and of r = 8 within 2^-40, u from 1e-4 to 14
    ub = np.array([t.u[i] for i, p in enumerate(pts) if p.family == "b" and p.tag.startswith("u=")])
    assert (ub < 0.5).any() and (ub > 0.5).any() and np.abs(ub / 0.5 - 1).min() < 2.0 ** -39
    rb = np.array([math.sqrt(p.L ** 2 - p.dH ** 2) / p.l for p in pts if p.family == "b" and p.tag.startswith("r=")])
    assert (rb < 8).any() and (rb > 8).any() and np.abs(rb / 8 - 1).min() < 2.0 ** -39
    ua = np.array([t.u[i] for i, p in enumerate(pts) if p.family == "a"])
    assert ua.min() < 2e-4 and ua.max() > 5.5 and (ua < 0.5).sum() > 50
    print("workspace: %d points, %s" % (len(pts), {f: len(v) for f, v in fam.items()}))


def test_root_residual():
    worst = 0.0
    for p in cr.workspace():
        root = cr.true_root(p.l, p.dH, p.L)
        if root is None:
            continue
        with mp.workdps(cr.DPS + 20):
            u = root[0]
            r = mp.sqrt(mpf(p.L) ** 2 - mpf(p.dH) ** 2) / mpf(p.l)
            res = abs(mp.sinh(u) - r * u) / mp.sinh(u)
            assert root[1] == 2 * u / mpf(p.l) or abs(root[1] * mpf(p.l) / (2 * u) - 1) < mpf(10) ** -45
        worst = max(worst, float(res))
        assert res < mpf("1e-40"), (p, float(res))
    print("largest root residual / sinh u = %.3g" % worst)


def test_no_root_inputs():
    assert cr.true_root(3.0, 4.0, 5.0) is None                       # exactly taut in doubles
    for p in cr.workspace():
        if p.family == "e":
            assert cr.true_root(p.l, p.dH, p.L) is None and cr.kappa(p.l, p.dH, p.L) == 0.0
    # kappa grows like 3 / u^2 near a taut horizontal cable
    l = 1.0
    for u in (1e-2, 1e-3):
        L = float(l * mp.sinh(mpf(u)) / mpf(u))
        us = float(cr.true_root(l, 0.0, L)[0])
        assert cr.kappa(l, 0.0, L) * us * us / 3 == pytest.approx(1.5, rel=1e-3)   # (1 + (L^2 + 0) / (2 L^2)) = 1.5


def test_margins_of_the_plain_reference():
    """m = max(4, 2 * largest ratio of brentq's error to eps (1 + kappa) |C*| + xtol); the reference itself stays within m / 2."""
    t = cr.table()
    ok = np.isfinite(t.C)
    assert np.isfinite(t.E_ref[ok]).all(), "brentq found no root at %s" % [t.pts[i] for i in np.nonzero(ok & ~np.isfinite(t.E_ref))[0]]
    rC, rT = cr.measured_margins()
    print("measured: largest ratio C %.3f (m = %.3g, recorded M_C = %g), tension %.3f (m = %.3g, recorded M_T = %g)"
          % (rC, max(4.0, 2 * rC), cr.M_C, rT, max(4.0, 2 * rT), cr.M_T))
    assert cr.M_C == pytest.approx(max(4.0, 2 * rC), rel=0.05) and cr.M_T == pytest.approx(max(4.0, 2 * rT), rel=0.05)
    ratio_C = t.E_ref[ok] / (t.scale_C[ok] + cr.XTOL)
    ratio_T = t.E_T_ref[ok] / (t.scale_T[ok] + t.xtol_T[ok])
    assert (ratio_C <= cr.M_C / 2).all() and (ratio_T <= cr.M_T / 2).all()
    bC, bT = cr.bounds()
    assert (t.E_ref[ok] <= bC[ok]).all() and (t.E_T_ref[ok] <= bT[ok]).all()


def test_fallback_tension_of_the_plain_reference(orc):
    """Every family (e) point: the oracle's tension with C = NaN is the w l / 2 the reference states."""
    t = cr.table()
    T, b = cr.expected_tension(*cr.C_WIDE)
    for i, p in enumerate(t.pts):
        if p.family != "e":
            continue
        with np.errstate(all="ignore"):
            To = float(orc.cable_tension(p.l, np.nan, p.L, cr.W_WET))
        if math.isfinite(T[i]):
            assert abs(To - T[i]) <= b[i], p
        else:
            assert (math.isnan(To) and math.isnan(T[i])) or To == T[i], p


@pytest.fixture(scope="module")
def shape_truth():
    return [cr.lowest_z_true((0.0, 0.0, 0.0), (rel[0], rel[1], up * rel[2]), th, ga, cr.L_WS, M, up, *cr.C_SHAPE)
            for rel, th, ga, M, up in cr.shape_cases()]


def test_lowest_point_margin(orc, shape_truth):
    cases = cr.shape_cases()
    assert len(cases) <= 120
    assert {c[3] for c in cases} == set(cr.MS) and {c[1] for c in cases} == set(cr.ANGLES) == {c[2] for c in cases}
    ratios = []
    for (rel, th, ga, M, up), tr in zip(cases, shape_truth):
        P = np.array([[rel[0], rel[1], up * rel[2]]])
        z = float(orc.augmented_lowest_z_vec(np.zeros(3), P, np.array([th]), np.array([ga]), cr.L_WS, M, up, *cr.C_SHAPE)[0])
        ratios.append(abs(float(mpf(z) - tr.z)) / cr.z_scale(tr.kappa))
    r = max(ratios)
    print("measured: largest ratio lowest point %.3f (m_z = %.3g, recorded M_Z = %g)" % (r, max(4.0, 2 * r), cr.M_Z))
    assert cr.M_Z == pytest.approx(max(4.0, 2 * r), rel=0.05)
    assert r <= cr.M_Z / 2
    # the cases the rollout's warm-started solve must meet: no root, a rejected warm start (r' >= cosh u_cold), u' < 0.5
    assert sum(not t.valid for t in shape_truth) >= 3
    assert sum(t.valid and t.u_cold is not None and t.r >= math.cosh(t.u_cold) for t in shape_truth) >= 3
    assert sum(t.valid and t.u < 0.5 for t in shape_truth) >= 3
    assert sum(t.valid and t.u_cold is not None and t.r < math.cosh(t.u_cold) for t in shape_truth) >= 3


def test_validity_rule():
    t = cr.table()
    for bracket in (cr.C_DEFAULT, cr.C_WIDE):
        valid, und = cr.validity(*bracket)
        assert und == [], [t.pts[i] for i in und]
    assert cr.validity(*cr.C_WIDE)[0].sum() == np.isfinite(t.C).sum()
    valid, und = cr.validity(*cr.C_NARROW)
    print("undecided on [%g, %g]: %s" % (cr.C_NARROW + ([t.pts[i] for i in und],)))
    assert len(und) <= 4 and all(t.pts[i].family == "c" and t.pts[i].tag.endswith("1e-9)") for i in und)
    # the narrow bracket cuts the workspace on both sides, and family (c) straddles both ends
    assert (t.C[np.isfinite(t.C)] < cr.C_NARROW[0]).any() and (t.C[np.isfinite(t.C)] > cr.C_NARROW[1]).any()
    for name in ("c_lo", "c_hi"):
        v = [bool(valid[i]) for i, p in enumerate(t.pts) if p.family == "c" and p.tag.startswith(name)]
        assert any(v) and not all(v)
