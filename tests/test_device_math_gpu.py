"""The hand-written math primitives of csrc/device_math.h, each by itself through rovmpc_math_probe, against the 50-digit
references of tests/device_math_reference.py.

Polynomial functions (trig kernels, exp increments, the two series, sinh_pos below 0.5): |got - ref| <= M * scale_i with the
scale and the margins M = (largest ratio of the correctly rounded restatement) + 1 of the reference module.  Functions seeded
by a hardware estimate: the bound device_math.h states, in ulp of the exact result (HW_BOUND).  Every test prints its
largest ratio before it asserts; profiles/device_math_probe.txt holds one run's figures.

sin(-0.0): the kernels give +0.0 where NumPy gives -0.0.  The deviation is kept and stated in include/rovmpc.h beside the
expression semantics; test_negative_zero pins it so that a change is noticed."""
import numpy as np
import pytest

import device_math_reference as dm

pytestmark = pytest.mark.gpu

FMTS = ("f64", "f32")
CHECKED_SIN = ("SIN", "SIN_PINNED")
PAIRS = ("SINCOS", "SINCOS_PINNED")


@pytest.fixture(scope="module")
def eng():
    import rovmpc
    with rovmpc.Engine(rovmpc.MPCConfig(N=1, K=1)) as e:
        yield e


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _cast(fmt, v):
    return np.asarray(v, dtype=np.float64).astype(dm.FMT[fmt].np).astype(np.float64)


def _ulp_ratio(got, ref, fmt):
    return dm.ratios(got, ref, dm.plain_scale(ref, dm.FMT[fmt]))


def _probe_trig(eng, fn, x, fmt):
    """(sin, cos or None)"""
    r = eng.math_probe(fn, x, dtype=fmt)
    return r if isinstance(r, tuple) else (r, None)


# ---- trig: the fast path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fn", CHECKED_SIN + ("SIN_BOUNDED",) + PAIRS)
def test_trig_fast_path(eng, fn, fmt):
    """Uniform in +-pi/2, +-100, +-1e6 (fp32: +-1e4), up to the limit, and the nearest representables to k pi/2 with both
    neighbours and both signs (k <= 64, 2^j and 2^j +- 1, 1024 random k): within M * scale."""
    x = dm.inputs_of("sin", fmt)
    s, c = _probe_trig(eng, fn, x, fmt)
    worst = {}
    for key, got in (("sincos_s", s), ("sincos_c", c)) if fn in PAIRS else (("sin", s),):
        ref, scale = dm.reference_of(key, fmt)
        ratio = dm.errors(got, ref) / scale
        for name, sl in dm.trig_slices(fmt).items():
            print("%s %s %s %-18s max error / scale %.3f  (M = %.3f, restatement %.3f)"
                  % (fn, fmt, key, name, ratio[sl].max(), dm.M(key, fmt), dm.MODEL_MAX[(key, fmt)]))
        worst[key] = (float(ratio.max()), dm.M(key, fmt), float(x[int(np.argmax(ratio))]))
    if fn == "SIN_BOUNDED":
        pinned = eng.math_probe("SIN_PINNED", x, dtype=fmt)
        assert np.array_equal(_bits(s), _bits(pinned)), "sin_bounded differs from the checked sine inside the limit"
    for key, (r, m, at) in worst.items():
        assert r <= m, (key, r, m, at)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fn", CHECKED_SIN + ("SIN_BOUNDED",) + PAIRS)
def test_trig_tiny_arguments_are_exact(eng, fn, fmt):
    """|x| < 2^-27 down to the denormals: sin x == x and cos x == 1 exactly."""
    x = dm.tiny_table(fmt)
    s, c = _probe_trig(eng, fn, x, fmt)
    bad = np.flatnonzero(_bits(s) != _bits(x))
    print("%s %s: %d tiny arguments, %d with sin x != x" % (fn, fmt, len(x), len(bad)))
    assert len(bad) == 0, (x[bad][:5], s[bad][:5])
    if c is not None:
        assert np.all(c == 1.0), x[c != 1.0][:5]


def _big_values(fmt):
    F = dm.FMT[fmt]
    big = [3e8, 1e10, 1e22] + ([1e300, float(np.finfo(np.float64).max)] if F is dm.F64 else [float(np.finfo(np.float32).max)])
    return _cast(fmt, big)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fn", CHECKED_SIN + PAIRS)
def test_trig_limit_and_beyond(eng, fn, fmt):
    """+-(limit - 1 ulp) is the last fast-path value, +-limit and everything above takes the library: fast lanes within
    M * scale, library lanes within 4 ulp of the reference (the OpenCL bound the device library is built to; this is about
    which lane gets which result, not about the library -- measured maxima: profiles/device_math_probe.txt, all below 1 ulp),
    inf and NaN give NaN."""
    F = dm.FMT[fmt]
    lf = dm.last_fast(F)
    big = _big_values(fmt)
    x = np.concatenate([[lf, -lf, F.limit, -F.limit], big, -big, [np.inf, -np.inf, np.nan]])
    s, c = _probe_trig(eng, fn, x, fmt)
    fast, lib = slice(0, 2), slice(2, 4 + 2 * len(big))
    for kind, got in (("sin", s), ("cos", c)):
        if got is None:
            continue
        key = "sin" if fn not in PAIRS else ("sincos_s" if kind == "sin" else "sincos_c")
        ref = dm.refs(kind, x[:lib.stop])
        scale = dm.trig_scale(x[fast], ref[fast], F, fn in PAIRS)
        rf = dm.errors(got[fast], ref[fast]) / scale
        rl = _ulp_ratio(got[lib], ref[lib], fmt)
        print("%s %s %s: last fast-path value error / scale %.3f (M = %.3f); at and above the limit max %.3f ulp (allowed %.0f)"
              % (fn, fmt, kind, rf.max(), dm.M(key, fmt), rl.max(), dm.LIBRARY_ULP))
        assert rf.max() <= dm.M(key, fmt), (kind, rf)
        assert rl.max() <= dm.LIBRARY_ULP, (kind, x[lib][rl > dm.LIBRARY_ULP], got[lib][rl > dm.LIBRARY_ULP])
        assert np.all(np.isnan(got[lib.stop:])), got[lib.stop:]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fn", CHECKED_SIN + PAIRS)
def test_trig_wave_mixing(eng, fn, fmt):
    """The large-argument branch is wave-uniform (one ballot), the selection per lane: whatever the wave holds, a small lane
    has the bits of the all-small launch and a big lane the bits of the all-big launch.  Arrangements: no big lane, all big,
    exactly one big lane at lane 0 / 31 / 63 of the first wave and in a later wave, a NaN lane among ordinary ones; n = 1, 63,
    65, 257 so that the last wave is partial."""
    F = dm.FMT[fmt]
    N = 257
    small = dm.trig_tables(fmt)["pm_100"][:N].copy()
    big = _cast(fmt, F.limit * (1.0 + np.arange(N) / 64.0))
    assert np.all(np.abs(small) < F.limit) and np.all(big >= F.limit) and len(set(big)) == N
    S = _probe_trig(eng, fn, small, fmt)
    B = _probe_trig(eng, fn, big, fmt)
    cases = 0
    for n in (1, 63, 65, 257):
        masks = {"none": [], "all": list(range(n))}
        for lane in (0, 31, 63, 64 + 31, 256):
            if lane < n:
                masks["one@%d" % lane] = [lane]
        for name, lanes in masks.items():
            m = np.zeros(n, bool); m[lanes] = True
            got = _probe_trig(eng, fn, np.where(m, big[:n], small[:n]), fmt)
            for g, s_, b_ in zip(got, S, B):
                if g is not None:
                    ok = _same_bits(g, np.where(m, b_[:n], s_[:n]))
                    assert ok.all(), (fn, fmt, n, name, np.flatnonzero(~ok))
            cases += 1
        for lane in (l for l in (0, 5, 63, 64) if l < n):
            x = small[:n].copy(); x[lane] = np.nan
            got = _probe_trig(eng, fn, x, fmt)
            for g, s_ in zip(got, S):
                if g is not None:
                    want = s_[:n].copy(); want[lane] = np.nan
                    assert _same_bits(g, want).all(), (fn, fmt, n, "nan@%d" % lane)
            cases += 1
    print("%s %s: %d arrangements, every lane bit-equal to its all-small / all-big launch" % (fn, fmt, cases))


@pytest.mark.parametrize("fmt", FMTS)
def test_negative_zero(eng, fmt):
    """sin(-0.0) is +0.0 on every trig kernel (fma(-k, P_hi, x) with k = -0 is (+0) P_hi + (-0) = +0), where NumPy gives
    -0.0: the stated deviation (include/rovmpc.h).  sin(+0.0) = +0.0 and cos(+-0.0) = 1 as everywhere."""
    z = np.array([-0.0, 0.0])
    for fn in CHECKED_SIN + ("SIN_BOUNDED",) + PAIRS:
        s, c = _probe_trig(eng, fn, z, fmt)
        print("%s %s: sin(-0.0) = %r, sin(+0.0) = %r" % (fn, fmt, s[0], s[1]))
        assert np.array_equal(_bits(s), _bits(np.array([0.0, 0.0]))), (fn, s)
        if c is not None:
            assert np.all(c == 1.0)


# ---- quotients ---------------------------------------------------------------------------------------------------------------
SPECIAL = [(1.0, 0.0), (-2.5, 0.0), (0.0, 0.0), (3.0, np.inf), (-3.0, -np.inf), (np.inf, 2.0), (np.nan, 1.0), (1.0, np.nan),
           (np.inf, np.inf), (0.0, 5.0), (-0.0, 5.0), (1.0, -0.0)]
EXTREME = [(1e300, 1e-300), (1e-300, 1e300), (3.0, 1e-310), (1e308, 1e308), (2e-308, 4.0), (1e200, 1e-200), (-7e305, 1e-10),
           (1e-320, 1e-320), (5e150, 2e160), (1.0, 1e308), (1e308, 0.5)]


def _np_div(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)


def _guard_pairs(n, seed):
    """Operand pairs log-uniform over the inside of m_divx's guard: |a| < 2^500, 2^-500 < |b| < 2^500."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(1, 2, n) * 2.0 ** rng.integers(-500, 500, n) * rng.choice([-1.0, 1.0], n)
    b = rng.uniform(1, 2, n) * 2.0 ** rng.integers(-499, 500, n) * rng.choice([-1.0, 1.0], n)
    assert np.all(np.abs(a) < 2.0 ** 500) and np.all(np.abs(b) > 2.0 ** -500) and np.all(np.abs(b) < 2.0 ** 500)
    return a, b


def test_divx_special_and_extreme_operands(eng):
    """m_divx on the special and extreme lists of test_expression_division_keeps_numpy_special_cases, |b| = 2^-500 and 2^500
    and |a| = 2^500 exactly and one ulp either side (both sides of the guard), a denormal a, quotients that land in the
    denormals: bit-equal to NumPy's a / b, signs of zero and inf included."""
    edge = lambda v: [float(np.nextafter(v, 0)), v, float(np.nextafter(v, np.inf))]
    pairs = list(SPECIAL) + list(EXTREME)
    for a in (1.0, -3.0, 7.5, 2.0 ** 499, 1e-200):
        pairs += [(a, sg * b) for v in (2.0 ** -500, 2.0 ** 500) for b in edge(v) for sg in (1.0, -1.0)]
    for b in (1.0, -3.0, 2.0 ** -499, 2.0 ** 499 * 1.5):
        pairs += [(sg * a, b) for a in edge(2.0 ** 500) for sg in (1.0, -1.0)]
    pairs += [(5e-324, 3.0), (1e-310, 2.0 ** -400), (-2.5e-315, 7.0), (5e-324, 5e-324), (1e-300, 1e100), (-1e-200, 1e120),
              (3e-308, 1e10), (1e-160, -1e160), (1e-320, 1e10), (2.0 ** -1022, 3.0)]
    a = np.array([p[0] for p in pairs]); b = np.array([p[1] for p in pairs])
    got = eng.math_probe("DIVX", a, b)
    want = _np_div(a, b)
    ok = _same_bits(got, want)
    print("DIVX f64: %d special / extreme pairs, %d not bit-equal to NumPy: %s"
          % (len(pairs), int((~ok).sum()), [(a[i], b[i], got[i], want[i]) for i in np.flatnonzero(~ok)]))
    assert ok.all()


@pytest.mark.parametrize("fn", ["DIVX", "DIVQ", "DIV"])
def test_fp64_quotient_inside_the_guard(eng, fn):
    """4096 operand pairs log-uniform over the guard's inside: within 1 ulp of the exact quotient."""
    a, b = _guard_pairs(4096, 11)
    got = eng.math_probe(fn, a, b)
    r = _ulp_ratio(got, dm.quotients(a, b), "f64")
    print("%s f64: max %.3f ulp over %d pairs inside the guard (bound %.0f), %d not correctly rounded"
          % (fn, r.max(), len(a), dm.HW_BOUND[(fn, "f64")], int((got != _np_div(a, b)).sum())))
    assert r.max() <= dm.HW_BOUND[(fn, "f64")]


@pytest.mark.parametrize("fn", ["DIVQ", "DIV"])
def test_fp64_quotient_special_operands(eng, fn):
    """a = 0, b = 0, +-inf and NaN: as IEEE (v_div_fixup), bit for bit."""
    vals = [0.0, -0.0, 1.5, -2.0, np.inf, -np.inf, np.nan]
    pairs = [(p, q) for p in vals for q in vals if not (np.isfinite(p) and np.isfinite(q) and p != 0 and q != 0)]
    a = np.array([p for p, _ in pairs]); b = np.array([q for _, q in pairs])
    got = eng.math_probe(fn, a, b)
    ok = _same_bits(got, _np_div(a, b))
    print("%s f64: %d special pairs, %d not as IEEE" % (fn, len(pairs), int((~ok).sum())))
    assert ok.all(), [(a[i], b[i], got[i]) for i in np.flatnonzero(~ok)]


def test_fp32_div(eng):
    """m_div in fp32 is a * v_rcp_f32(b): 1 ulp of the reciprocal, then one rounding of the product -- 2 ulp, for operands of
    order 1e-6 to 1e6."""
    rng = np.random.default_rng(12)
    a = _cast("f32", 10.0 ** rng.uniform(-6, 6, 4096) * rng.choice([-1.0, 1.0], 4096))
    b = _cast("f32", 10.0 ** rng.uniform(-6, 6, 4096) * rng.choice([-1.0, 1.0], 4096))
    got = eng.math_probe("DIV", a, b, dtype="f32")
    r = _ulp_ratio(got, dm.quotients(a, b), "f32")
    print("DIV f32: max %.3f ulp over %d pairs (bound %.0f)" % (r.max(), len(a), dm.HW_BOUND[("DIV", "f32")]))
    assert r.max() <= dm.HW_BOUND[("DIV", "f32")]


# ---- roots and reciprocals ---------------------------------------------------------------------------------------------------
def _sqrtq_worst(eng, tables):
    worst = {}
    for name, x in tables.items():
        r = _ulp_ratio(eng.math_probe("SQRTQ", x), dm.refs("sqrt", x), "f64")
        worst[name] = (float(r.max()), float(x[int(np.argmax(r))]))
        print("SQRTQ f64 %-24s max %.3f ulp (bound %.0f)" % (name, r.max(), dm.HW_BOUND[("SQRTQ", "f64")]))
    return worst


def test_sqrtq(eng):
    """m_sqrtq: 0 -> 0, -0 -> -0, inf -> inf, NaN and negatives -> NaN; 2^-1022, DBL_MAX, 4096 inputs log-uniform over the
    whole normal range and the rollout's squared norms (1e-6 .. 1e10): within 1 ulp."""
    sp = np.array([0.0, -0.0, np.inf, np.nan, -1.0, -1e-300, -np.inf, -5e-324])
    got = eng.math_probe("SQRTQ", sp)
    assert np.array_equal(_bits(got[:3]), _bits(sp[:3])), got[:3]
    assert np.all(np.isnan(got[3:])), got[3:]
    rng = np.random.default_rng(13)
    tables = {
        "edges": np.array([2.0 ** -1022, float(np.finfo(np.float64).max), 1.0, 2.0, 4.0, float(np.nextafter(4.0, 0))]),
        "whole range": rng.uniform(1, 2, 4096) * 2.0 ** rng.integers(-1022, 1024, 4096),
        "rollout (1e-6 .. 1e10)": 10.0 ** rng.uniform(-6, 10, 2048),
    }
    for name, (r, at) in _sqrtq_worst(eng, tables).items():
        assert r <= dm.HW_BOUND[("SQRTQ", "f64")], (name, r, at)


def test_sqrtq_denormal_inputs(eng):
    """Denormal x, 5e-324 up to the last value below 2^-1022: within 1 ulp.

    This test found a defect: with the residual x - g^2 formed at x's own scale it is, for a denormal x, a multiple of 2^-1074
    with a handful of bits or none, and the result was the uncorrected Goldschmidt iterate, 10.698 ulp at x = 2.5867744e-316
    (MI355X).  m_sqrtq now forms the residual 2^128 up for those lanes (device_math.h): 0.497 ulp here, no other bit changed."""
    rng = np.random.default_rng(13)
    tables = {"denormals": np.concatenate([[5e-324, 1e-323, 2.0 ** -1023, float(np.nextafter(2.0 ** -1022, 0))], 2.0 ** rng.uniform(-1074, -1022, 252)])}
    assert np.all(tables["denormals"] < 2.0 ** -1022)
    for name, (r, at) in _sqrtq_worst(eng, tables).items():
        assert r <= dm.HW_BOUND[("SQRTQ", "f64")], (name, r, at)


def test_fp32_sqrt(eng):
    """m_sqrt in fp32 is v_sqrt_f32: 1 ulp over the normal range, 0 -> 0, -0 -> -0, inf -> inf, NaN and negatives -> NaN.
    Denormal inputs: the instruction reads them as zero, whatever the kernel's denormal mode (measured: every one of 2^-149
    .. 2^-126 (1 - 2^-23) gives +0.0, where the root is up to 1.08e-19) -- pinned here as it is; the fp32 kernels take roots
    of squared norms and of L^2 - dH^2, which are zero or far above 1e-38."""
    rng = np.random.default_rng(14)
    x = _cast("f32", np.concatenate([rng.uniform(1, 2, 2048) * 2.0 ** rng.integers(-126, 128, 2048), [2.0 ** -126, float(np.finfo(np.float32).max), 1.0, 4.0]]))
    r = _ulp_ratio(eng.math_probe("SQRT", x, dtype="f32"), dm.refs("sqrt", x), "f32")
    print("SQRT f32 normal range: max %.3f ulp (bound %.0f)" % (r.max(), dm.HW_BOUND[("SQRT", "f32")]))
    sp = np.array([0.0, -0.0, np.inf, np.nan, -1.0, -np.inf])
    got = eng.math_probe("SQRT", sp, dtype="f32")
    den = _cast("f32", np.concatenate([[2.0 ** -149, 2.0 ** -148, 2.0 ** -127, float(np.nextafter(np.float32(2.0 ** -126), np.float32(0)))],
                                       2.0 ** rng.uniform(-149, -126, 252)]))
    assert np.all((den > 0) & (den < 2.0 ** -126))
    gd = eng.math_probe("SQRT", den, dtype="f32")
    print("SQRT f32 denormal inputs: %d of %d give +0.0; sqrt(2^-149) = %r" % (int((_bits(gd) == 0).sum()), len(den), gd[0]))
    assert r.max() <= dm.HW_BOUND[("SQRT", "f32")]
    assert np.array_equal(_bits(got[:3]), _bits(sp[:3])) and np.all(np.isnan(got[3:])), got
    assert np.all(_bits(gd) == 0), (den[_bits(gd) != 0][:5], gd[_bits(gd) != 0][:5])


@pytest.mark.parametrize("fmt", FMTS)
def test_rcp(eng, fmt):
    """fast_rcp: [2^-1000, 2^1000] log-uniform and the rollout's [1e-8, 1e8] densely (fp32: v_rcp_f32 on [2^-100, 2^100] and
    the same dense range), within 1 ulp; NaN and inf give a non-finite result (what cable_tension's caller relies on)."""
    rng = np.random.default_rng(15)
    e = 1000 if fmt == "f64" else 100
    tables = {"log-uniform 2^+-%d" % e: rng.uniform(1, 2, 2048) * 2.0 ** rng.integers(-e, e, 2048),
              "rollout (1e-8 .. 1e8)": 10.0 ** rng.uniform(-8, 8, 4096)}
    worst = {}
    for name, x in tables.items():
        x = _cast(fmt, x)
        r = _ulp_ratio(eng.math_probe("RCP", x, dtype=fmt), dm.refs("rcp", x), fmt)
        worst[name] = float(r.max())
        print("RCP %s %-22s max %.3f ulp (bound 1)" % (fmt, name, r.max()))
    if fmt == "f64":
        got = eng.math_probe("RCP", np.array([np.nan, np.inf, -np.inf]), dtype=fmt)
        print("RCP f64 of NaN, inf, -inf: %s" % got)
        assert not np.isfinite(got).any(), got
    for name, r in worst.items():
        assert r <= 1.0, (name, r)


@pytest.mark.parametrize("fmt", FMTS)
def test_min_raw(eng, fmt):
    """v_min: a NaN on either side returns the other operand, two NaNs a NaN, ordinary pairs np.fmin."""
    rng = np.random.default_rng(16)
    a = _cast(fmt, np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-20, 20, 500), [np.nan, 3.0, np.nan, np.inf, -np.inf, np.nan, 1.0, -0.0]]))
    b = _cast(fmt, np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-20, 20, 500), [2.0, np.nan, np.nan, 1.0, np.nan, -np.inf, 1.0, -0.0]]))
    got = eng.math_probe("MIN_RAW", a, b, dtype=fmt)
    ok = _same_bits(got, np.fmin(a, b))
    print("MIN_RAW %s: %d pairs, %d differ from np.fmin" % (fmt, len(a), int((~ok).sum())))
    assert ok.all(), [(a[i], b[i], got[i]) for i in np.flatnonzero(~ok)]


# ---- the short polynomials of the cable solve ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fn,key", [("EXP_INC", "exp_inc"), ("EXP_INC_TINY", "exp_inc_tiny"), ("SINHC_M1_SMALL", "sinhc"),
                                    ("COSH_M1_SMALL", "coshc"), ("SINH_POS", "sinh_small")])
def test_cable_polynomials(eng, fn, key, fmt):
    """exp_increment on |d| < 2^-5 (+-2^-5 (1 - eps) and the denormals included), exp_increment_tiny on |d| < 2^-15, the two
    series on the squares of x in [0, 0.5), sinh_pos on [0, 0.5): within M ulp of the reference (relative: the results of the
    series are small)."""
    x = dm.inputs_of(key, fmt)
    ref, scale = dm.reference_of(key, fmt)
    got = eng.math_probe(fn, x, dtype=fmt)
    ratio = dm.errors(got, ref) / scale
    print("%s %s: max error / ulp %.3f over %d inputs (M = %.3f, restatement %.3f)"
          % (fn, fmt, ratio.max(), len(x), dm.M(key, fmt), dm.MODEL_MAX[(key, fmt)]))
    assert ratio.max() <= dm.M(key, fmt), (float(ratio.max()), float(x[int(np.argmax(ratio))]))


@pytest.mark.parametrize("fmt", FMTS)
def test_sinh_pos_exponential_form(eng, fmt):
    """sinh_pos on [0.5, 40] (0.5 itself and the next value included) is (e - 1 / e) / 2 with the library's exp: within the
    first-order running error bound of that form for an exp good to 1 ulp (dm.sinh_big_bound)."""
    x = dm.poly_tables(fmt)["sinh_big"]
    ref = dm.refs("sinh", x)
    bound = dm.sinh_big_bound(x, dm.FMT[fmt])
    got = eng.math_probe("SINH_POS", x, dtype=fmt)
    err = dm.errors(got, ref)
    print("SINH_POS %s on [0.5, 40]: max error / running bound %.3f, max %.3f ulp" % (fmt, (err / bound).max(), _ulp_ratio(got, ref, fmt).max()))
    assert np.all(err <= bound), (x[err > bound][:5], (err / bound).max())


# ---- the probe measures what loaded models run ------------------------------------------------------------------------------------
def test_expressions_run_the_probed_functions(eng):
    """sin(x0), cos(x0) and x0 / x1 through eval_expression (the interpreter of loaded models) are bit-equal to the probe's
    SIN, the cosine of SINCOS and DIVX on the trig and division tables."""
    from rovmpc import expr as E
    x = np.concatenate([dm.inputs_of("sin", "f64"), dm.tiny_table("f64"), _big_values("f64"), [dm.last_fast(dm.F64), dm.F64.limit, -0.0, np.nan, np.inf]])
    a, b = _guard_pairs(4096, 11)
    a = np.concatenate([a, [p for p, _ in SPECIAL + EXTREME]]); b = np.concatenate([b, [q for _, q in SPECIAL + EXTREME]])
    consts = []
    X = np.zeros((len(x), 2)); X[:, 0] = x
    s = eng.eval_expression(E.compile_expression("sin(x0)", consts, 2).code, consts, X)
    c = eng.eval_expression(E.compile_expression("cos(x0)", consts, 2).code, consts, X)
    q = eng.eval_expression(E.compile_expression("x0 / x1", consts, 2).code, consts, np.column_stack([a, b]))
    assert consts == []
    ok_s = _same_bits(s, eng.math_probe("SIN", x))
    ok_c = _same_bits(c, eng.math_probe("SINCOS", x)[1])
    ok_q = _same_bits(q, eng.math_probe("DIVX", a, b))
    print("expression vs probe: sin %d / %d, cos %d / %d, x0 / x1 %d / %d bit-equal"
          % (ok_s.sum(), len(x), ok_c.sum(), len(x), ok_q.sum(), len(a)))
    assert ok_s.all() and ok_c.all() and ok_q.all()


def test_probe_refuses_what_it_cannot_run(eng):
    """The unchecked sine is undefined at or above its limit: such inputs (and non-finite ones) are refused before a launch."""
    import rovmpc
    for fmt in FMTS:
        F = dm.FMT[fmt]
        assert len(eng.math_probe("SIN_BOUNDED", [dm.last_fast(F), -dm.last_fast(F)], dtype=fmt)) == 2
        for bad in (F.limit, -F.limit, 1e300, np.inf, -np.inf, np.nan):
            with pytest.raises(rovmpc.RovmpcError) as ei:
                eng.math_probe("SIN_BOUNDED", [0.5, bad], dtype=fmt)
            assert ei.value.code == -1
    with pytest.raises(ValueError):
        eng.math_probe("NO_SUCH", [1.0])
    with pytest.raises(ValueError):
        eng.math_probe("DIVX", [1.0])
    assert len(eng.math_probe("SIN", [])) == 0
