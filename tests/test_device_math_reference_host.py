"""CPU checks of tests/device_math_reference.py: the rounding model against NumPy's own arithmetic, the 50-digit references
against identities, the margins MODEL_MAX reproducing, and the sensitivity of the asserted bounds M * scale to a subtly
wrong kernel (on the restatement: no GPU here)."""
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import device_math_reference as dm

CASES = [(k, f) for f in ("f64", "f32") for k in dm.POLY]


def test_rounding_model_is_numpy_arithmetic():
    """rnd() on exact products and sums gives what NumPy's correctly rounded * and + give, in both types, denormals included."""
    rng = np.random.default_rng(1)
    for F in (dm.F64, dm.F32):
        a = (rng.standard_normal(300) * 10.0 ** rng.integers(-8, 8, 300)).astype(F.np)
        b = (rng.standard_normal(300) * 10.0 ** rng.integers(-8, 8, 300)).astype(F.np)
        tiny = F.np(2.0 ** (F.emin + 3))
        for x, y in list(zip(a, b)) + [(tiny, F.np(0.3)), (tiny, F.np(2.0 ** -5)), (F.np(1.5), F.np(2.0 ** F.emin))]:
            fx, fy = Fraction(float(x)), Fraction(float(y))
            assert float(dm.mul(fx, fy, F)) == float(x * y)
            assert float(dm.add(fx, fy, F)) == float(x + y)
    assert dm.rint(Fraction(5, 2)) == 2 and dm.rint(Fraction(7, 2)) == 4 and dm.rint(Fraction(-5, 2)) == -2
    # a decimal literal read into T, and fma with a single rounding (the product alone would round the low part away)
    assert float(dm.lit("3.14159274", dm.F32)) == float(np.float32(3.14159274))
    assert float(dm.lit("1.22464679914735317723e-16", dm.F64)) == 1.22464679914735317723e-16
    e = Fraction(2) ** -30
    assert dm.fma(1 + e, 1 - e, Fraction(-1), dm.F64) == -e * e and dm.add(dm.mul(1 + e, 1 - e, dm.F64), -1, dm.F64) == 0


def test_reduction_constants_split_pi():
    """P_hi + P_lo is pi (pi / 2) to half an ulp of P_lo, the premise of the error scale; inv is the rounded reciprocal."""
    with mp.workdps(dm.DPS):
        for F in (dm.F64, dm.F32):
            for K, P in ((dm.sin_constants(F), mp.pi), (dm.sincos_constants(F), mp.pi / 2)):
                gap = abs(dm._mpf(K["hi"]) + dm._mpf(K["lo"]) - P)
                assert gap <= 0.5 * float(dm.ulp(float(K["lo"]), F))
                assert float(K["hi"]) == float(F.np(float(P))) and float(K["inv"]) == float(F.np(float(1 / P)))


def test_references_satisfy_identities():
    with mp.workdps(dm.DPS):
        for x2 in (Fraction(1, 4), Fraction(1, 10 ** 30), Fraction(3, 100)):
            with mp.workdps(3 * dm.DPS):                # (the closed forms cancel: 30 digits are lost at x2 = 1e-30)
                x = mp.sqrt(dm._mpf(x2))
                direct_s, direct_c = mp.sinh(x) / x - 1, mp.cosh(x) - 1
            assert abs(dm.ref_sinhc_m1(x2) / direct_s - 1) < mp.mpf(10) ** -45
            assert abs(dm.ref_cosh_m1(x2) / direct_c - 1) < mp.mpf(10) ** -45
        assert dm.ref_sinhc_m1(0.0) == 0 and dm.ref_cosh_m1(0.0) == 0
        for x in (0.25, 0.4999, 0.5, 3.0):
            assert abs(dm.ref_sinh(x) / mp.sinh(mp.mpf(x)) - 1) < mp.mpf(10) ** -45
        s, c = dm.refs("sin", [1e22])[0], dm.refs("cos", [1e22])[0]
        assert abs(s * s + c * c - 1) < mp.mpf(10) ** -45 and abs(float(s) - -0.8522008497671888) < 1e-15
    q = dm.quotients([1.0, 1e-300], [3.0, 1e100])
    assert float(q[0]) == 1.0 / 3.0 and float(q[1]) == 1e-300 / 1e100


def test_tables_cover_what_they_claim():
    for fmt, F in dm.FMT.items():
        t = dm.trig_tables(fmt)
        assert all(len(v) <= 7000 for v in t.values())
        k = np.rint(t["near_kpio2"] / (np.pi / 2))
        assert set(range(1, 65)) <= set(np.abs(k).astype(int)) and {int(v) % 4 for v in np.abs(k)} == {0, 1, 2, 3}
        assert np.abs(t["to_limit"]).max() > 0.95 * F.limit and np.abs(t["near_kpio2"]).max() > 0.49 * F.limit
        assert dm.last_fast(F) < F.limit and float(F.np(dm.last_fast(F))) == dm.last_fast(F)
        ty = dm.tiny_table(fmt)
        assert np.abs(ty).min() == 2.0 ** (F.emin - F.p + 1) and (ty < 0).any() and (ty > 0).any()
        p = dm.poly_tables(fmt)
        assert np.abs(p["exp_inc"]).max() == 2.0 ** -5 * (1 - 2.0 ** -F.p) and np.abs(p["exp_inc_tiny"]).max() < 2.0 ** -15
        assert p["series_x2"].max() < 0.25 and p["sinh_small"].max() < 0.5 and p["sinh_big"].min() == 0.5
        assert set(dm.trig_slices(fmt)) == set(t)


@pytest.mark.parametrize("fmt", ["f64", "f32"])
def test_sinh_running_bound_holds_for_a_correctly_rounded_exp(fmt):
    """(e - 1 / e) / 2 with e the correctly rounded exponential and each operation rounded once lies within sinh_big_bound
    (which allows a whole ulp on e), and the bound is nowhere looser than 4 ulp of the result (3.5 just above x = ln 2: e in [2, 4) has four times the ulp of the result in [0.5, 1))."""
    F = dm.FMT[fmt]
    x = dm.poly_tables(fmt)["sinh_big"][::4]
    got = []
    with mp.workdps(dm.DPS):
        for v in x:
            t = mp.exp(mp.mpf(float(v)))
            e = dm.rnd(Fraction(int(mp.floor(mp.ldexp(t, 200))), 2 ** 200), F)
            got.append(dm.add(e, -dm.rnd(1 / e, F), F) / 2)
    ref = dm.refs("sinh", x)
    bound = dm.sinh_big_bound(x, F)
    assert np.all(dm.errors(got, ref) <= bound)
    assert np.all(bound <= 4.0 * dm.plain_scale(ref, F))


@pytest.mark.parametrize("key,fmt", CASES, ids=["%s-%s" % c for c in CASES])
def test_margin_reproduces(key, fmt):
    """MODEL_MAX is what the restatement gives on the test's own inputs (both contraction extremes), and no bound M * scale
    exceeds DESIGN.md's "few": 4."""
    got = dm.model_ratio(key, fmt)
    print("%s %s: restatement max error / scale %.4f (recorded %.3f), M = %.3f" % (key, fmt, got, dm.MODEL_MAX[(key, fmt)], dm.M(key, fmt)))
    assert abs(got - dm.MODEL_MAX[(key, fmt)]) <= 1e-3
    assert dm.M(key, fmt) <= 4.0


@pytest.mark.parametrize("key,fmt", CASES, ids=["%s-%s" % c for c in CASES])
def test_bounds_notice_a_perturbed_constant(key, fmt):
    """Each polynomial coefficient off by 1e-3 relative, *_hi off by an ulp, *_lo off by 2^-20 relative: the restatement then
    exceeds M * scale on the test's inputs -- except for the perturbations UNDETECTED names, which do at the size it names."""
    make = dm.perturbations(key, fmt)
    idx = dm.perturbation_subset(key, fmt)
    names = list(make(1))
    assert names and {n for (k, f, n) in dm.UNDETECTED if (k, f) == (key, fmt)} <= set(names)
    for name in names:
        r = dm.model_ratio(key, fmt, make(1)[name], idx)
        if (key, fmt, name) not in dm.UNDETECTED:
            assert r > dm.M(key, fmt), (name, r)
            continue
        assert r <= dm.M(key, fmt), (name, r, "is detected: take it out of UNDETECTED")
        size = dm.UNDETECTED[(key, fmt, name)]
        if size is not None:
            assert dm.model_ratio(key, fmt, make(size)[name], idx) > dm.M(key, fmt), (name, size)
            assert dm.model_ratio(key, fmt, make(size // 4)[name], idx) <= dm.M(key, fmt), (name, size)
