"""The hand-written device math of csrc/device_math.h against 50-digit mpmath: reference values, the input tables of
tests/test_device_math_gpu.py, the per-point error scale, and a correctly rounded restatement of the polynomial kernels.

Error scale.  A result is measured in units of scale_i:

  trig kernels        scale_i = ulp_T(ref_i) + (|x_i| / P) * 1/2 ulp_T(P_lo)
  everything else     scale_i = ulp_T(ref_i)

Below the fast-path limit the first reduction FMA x - k P_hi is exact and the second rounds once (within 1/2 ulp of the
reduced argument); the one error that grows with the argument is the rounding of the low reduction constant itself,
|P - (P_hi + P_lo)| <= 1/2 ulp_T(P_lo), taken k ~ |x| / P times.  (P, P_lo) is (pi, pi_lo) for the sine-alone kernels and
(pi/2, pio2_lo) for the pairs.  Next to a multiple of pi/2 the raw error is hundreds of ulp of the (tiny) reference while
error / scale stays where it is at generic points.

Margins.  The bound a GPU test asserts for a polynomial function is M * scale_i with M = MODEL_MAX + 1: MODEL_MAX is the
largest error / scale of the restatement below (every fma, * and + rounded once to T, built on fractions.Fraction) over
the test's own inputs, at both contraction extremes where the source leaves a * b + c to the compiler (the Horner forms of
fast_sincos_k, the series under `fp contract(on)`); the added 1 is for rounding choices of the compiler the model cannot
know.  tests/test_device_math_reference_host.py measures MODEL_MAX again and fails if the constants no longer reproduce,
and shows on the restatement that the bounds notice a coefficient off by 1e-3, a *_hi constant off by an ulp and a *_lo
constant off by 2^-20 (UNDETECTED names the perturbations the inputs cannot see, with the size at which they do).

Functions seeded by a hardware estimate (v_rcp, v_rsq, v_sqrt_f32) cannot be restated: their bound is the statement in
device_math.h, HW_BOUND, in ulp of the exact result."""
from fractions import Fraction
from functools import lru_cache

import mpmath as mp
import numpy as np

DPS = 50


# ---- number formats ---------------------------------------------------------------------------------------------------
class Fmt:
    def __init__(self, name, p, emin, np_type, limit):
        self.name, self.p, self.emin, self.np, self.limit = name, p, emin, np_type, limit

    def __repr__(self):
        return self.name


F64 = Fmt("f64", 53, -1022, np.float64, 2.0 ** 26)         # limit: TRIG_FAST_LIMIT
F32 = Fmt("f32", 24, -126, np.float32, 32768.0)            # limit: TRIGF_FAST_LIMIT
FMT = {"f64": F64, "f32": F32}


def rnd(q, F):
    """The Fraction q rounded once, to nearest even, to format F (denormals included; no overflow in this module)."""
    n, d = q.numerator, q.denominator
    if n == 0:
        return q
    an = abs(n)
    e = an.bit_length() - d.bit_length()
    if (an << max(0, -e)) < (d << max(0, e)):
        e -= 1                                              # 2^e <= |q| < 2^(e+1)
    sh = max(e, F.emin) - (F.p - 1)
    num, den = (an, d << sh) if sh >= 0 else (an << -sh, d)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and m & 1):
        m += 1
    if n < 0:
        m = -m
    return Fraction(m << sh) if sh >= 0 else Fraction(m, 1 << -sh)


def fma(a, b, c, F):
    return rnd(a * b + c, F)


def mul(a, b, F):
    return rnd(a * b, F)


def add(a, b, F):
    return rnd(a + b, F)


def rint(q):
    return Fraction(round(q))                               # half to even, as v_rndne


def lit(s, F):
    """A decimal literal of the source as the compiler reads it into T."""
    return rnd(Fraction(s), F)


def ulp(v, F):
    """One unit in the last place of |v| in F (v: float or array)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(F.np)).astype(np.float64)


# ---- constants of device_math.h (trig_constants, sin_constants, fast_sinf_k, fast_sincosf_k) ---------------------------
def sincos_constants(F):
    """(inv_pio2, pio2_hi, pio2_lo, S[...], C[...])"""
    if F is F64:
        t = ["6.36619772367581382433e-01", "1.57079632679489655800e+00", "6.12323399573676603587e-17"]
        S = ["-1.66666666666666324348e-01", "8.33333333332248946124e-03", "-1.98412698298579493134e-04",
             "2.75573137070700676789e-06", "-2.50507602534068634195e-08", "1.58969099521155010221e-10"]
        Cc = ["4.16666666666666019037e-02", "-1.38888888888741095749e-03", "2.48015872894767294178e-05",
              "-2.75573143513906633035e-07", "2.08757232129817482790e-09", "-1.13596475577881948265e-11"]
    else:
        t = ["0.636619772", "1.57079637", "-4.37113883e-8"]
        S = ["-0.16666667", "0.0083333294", "-0.00019839335", "2.7183114e-06"]
        Cc = ["0.041666623", "-0.0013886764", "2.4390449e-05"]
    return {"inv": lit(t[0], F), "hi": lit(t[1], F), "lo": lit(t[2], F), "S": [lit(s, F) for s in S], "C": [lit(s, F) for s in Cc]}


def sin_constants(F):
    """(inv_pi, pi_hi, pi_lo, c[...])"""
    if F is F64:
        t = ["0.31830988618379067154", "3.14159265358979311600e+00", "1.22464679914735317723e-16"]
        c = ["-0.16666666666666666", "0.008333333333333316", "-0.00019841269841254885", "2.7557319219139174e-06",
             "-2.5052107613933993e-08", "1.6058977114025027e-10", "-7.643963964341869e-13", "2.7313658477694193e-15"]
    else:
        t = ["0.318309886", "3.14159274", "-8.74227766e-8"]
        c = ["-0.16666666", "0.008333237", "-0.00019822021", "2.6324394e-06"]
    return {"inv": lit(t[0], F), "hi": lit(t[1], F), "lo": lit(t[2], F), "c": [lit(s, F) for s in c]}


# ---- the kernels restated (x and every result a Fraction that T holds exactly) ------------------------------------------
def model_sin(x, F, K=None, fused=True):
    """fast_sin_k (fp64: Estrin) / fast_sinf_k (fp32: Horner) below the limit.  Every a * b + c is an explicit fma in the source."""
    K = K or sin_constants(F)
    c = K["c"]
    k = rint(mul(x, K["inv"], F))
    r = fma(-k, K["hi"], x, F)
    r = fma(-k, K["lo"], r, F)
    z = mul(r, r, F)
    if F is F64:
        z2 = mul(z, z, F)
        z4 = mul(z2, z2, F)
        p01, p23, p45, p67 = (fma(c[2 * i + 1], z, c[2 * i], F) for i in range(4))
        p = fma(fma(p67, z2, p45, F), z4, fma(p23, z2, p01, F), F)
    else:
        p = fma(z, c[3], c[2], F)
        p = fma(z, p, c[1], F)
        p = fma(z, p, c[0], F)
    v = fma(mul(r, z, F), p, r, F)
    return -v if int(k) & 1 else v


def model_sincos(x, F, K=None, fused=True):
    """fast_sincos_k / fast_sincosf_k below the limit.  fp64: the Horner forms and z z pc + (...) are plain a * b + c in the
    source (`fused` picks the contraction extreme); fp32: explicit fmaf throughout."""
    K = K or sincos_constants(F)
    S, Cc = K["S"], K["C"]
    k = rint(mul(x, K["inv"], F))
    r = fma(-k, K["hi"], x, F)
    r = fma(-k, K["lo"], r, F)
    z = mul(r, r, F)
    if F is F64:
        def horner(cs):
            acc = cs[-1]
            for cf in reversed(cs[:-1]):
                acc = fma(z, acc, cf, F) if fused else add(cf, mul(z, acc, F), F)
            return acc
        sr = fma(mul(z, r, F), horner(S), r, F)
        pc = horner(Cc)
        hz = mul(Fraction(1, 2), z, F)
        w = add(1, -hz, F)
        inner = add(add(1, -w, F), -hz, F)
        t = mul(z, z, F)
        inner = fma(t, pc, inner, F) if fused else add(inner, mul(t, pc, F), F)
        cr = add(w, inner, F)
    else:
        ps = fma(z, S[3], S[2], F)
        ps = fma(z, ps, S[1], F)
        ps = fma(z, ps, S[0], F)
        sr = fma(mul(r, z, F), ps, r, F)
        pc = fma(z, Cc[2], Cc[1], F)
        pc = fma(z, pc, Cc[0], F)
        cr = fma(mul(z, z, F), pc, fma(z, Fraction(-1, 2), Fraction(1), F), F)
    q = int(k)
    ss, cc = (cr, sr) if q & 1 else (sr, cr)
    return (-ss if q & 2 else ss), (-cc if (q + 1) & 2 else cc)


def _recip(n, F):
    """T(1.0 / n) of the source: the double quotient, then converted."""
    return rnd(rnd(Fraction(1, n), F64), F)


def exp_inc_constants(F):
    return [_recip(n, F) if F is F64 else rnd(Fraction(1, n), F) for n in ((5040, 720, 120, 24, 6, 2, 1) if F is F64 else (24, 6, 2, 1))]


def model_exp_inc(d, F, K=None, fused=True):
    """exp_increment: Horner in explicit fma, to d^7 (fp64) / d^4 (fp32)."""
    K = K or exp_inc_constants(F)
    if F is F64:
        p = K[0]
        for cf in K[1:]:
            p = fma(p, d, cf, F)
    else:
        p = fma(d, K[0], K[1], F)
        for cf in K[2:]:
            p = fma(p, d, cf, F)
    return fma(p, d, Fraction(1), F)


def exp_inc_tiny_constants(F):
    return [_recip(6, F), Fraction(1, 2)] if F is F64 else [Fraction(1, 2)]


def model_exp_inc_tiny(d, F, K=None, fused=True):
    K = K or exp_inc_tiny_constants(F)
    p = fma(d, K[0], K[1], F) if F is F64 else K[0]
    return fma(fma(p, d, Fraction(1), F), d, Fraction(1), F)


SINHC_DEN = (6, 20, 42, 72, 110, 156, 210, 272)
COSHC_DEN = (2, 12, 30, 56, 90, 132, 182, 240)


def series_constants(den, F):
    return [_recip(n, F) for n in den]


def _series(x2, F, K, fused):
    """x2 c1 (1 + x2 c2 (1 + ... (1 + x2 c8))): under `fp contract(on)` each 1 + (x2 c) * inner may become one fma."""
    inner = fma(x2, K[-1], Fraction(1), F) if fused else add(1, mul(x2, K[-1], F), F)
    for cf in reversed(K[1:-1]):
        t = mul(x2, cf, F)
        inner = fma(t, inner, Fraction(1), F) if fused else add(1, mul(t, inner, F), F)
    return mul(mul(x2, K[0], F), inner, F)


def model_sinhc(x2, F, K=None, fused=True):
    return _series(x2, F, K or series_constants(SINHC_DEN, F), fused)


def model_coshc(x2, F, K=None, fused=True):
    return _series(x2, F, K or series_constants(COSHC_DEN, F), fused)


def model_sinh_small(x, F, K=None, fused=True):
    """sinh_pos below 0.5: x (1 + S(x x)); the sum and the products stand in separate expressions (no contraction)."""
    return mul(x, add(1, model_sinhc(mul(x, x, F), F, K, fused), F), F)


# ---- 50-digit references ---------------------------------------------------------------------------------------------------
def _mpf(v):
    if isinstance(v, mp.mpf):
        return v
    return mp.mpf(v.numerator) / mp.mpf(v.denominator) if isinstance(v, Fraction) else mp.mpf(float(v))


def _taylor(x2, start, k0):
    """sum_{n >= 1} x2^n / (k0 + 2 n)!  -- all terms positive (no cancellation at any x2)."""
    term, total, n = start, mp.mpf(0), 0
    while True:
        n += 1
        term = term * x2 / ((k0 + 2 * n - 1) * (k0 + 2 * n))
        total += term
        if term <= total * mp.mpf(10) ** -(DPS + 5):
            return total


def ref_sinhc_m1(x2):
    """sinh(x) / x - 1 as a function of x2 = x^2."""
    x2 = _mpf(x2)
    return mp.mpf(0) if x2 == 0 else _taylor(x2, mp.mpf(1), 1)


def ref_cosh_m1(x2):
    x2 = _mpf(x2)
    return mp.mpf(0) if x2 == 0 else _taylor(x2, mp.mpf(1), 0)


def ref_sinh(x):
    x = _mpf(x)
    return x * (1 + ref_sinhc_m1(x * x)) if x < 0.5 else mp.sinh(x)


REF = {
    "sin": lambda x: mp.sin(_mpf(x)), "cos": lambda x: mp.cos(_mpf(x)), "exp": lambda x: mp.exp(_mpf(x)),
    "sinhc": ref_sinhc_m1, "coshc": ref_cosh_m1, "sinh": ref_sinh, "sqrt": lambda x: mp.sqrt(_mpf(x)),
    "rcp": lambda x: 1 / _mpf(x),
}


def refs(name, xs):
    """List of mpf references of REF[name] over xs (floats or Fractions)."""
    with mp.workdps(DPS + 10):
        return [REF[name](x) for x in xs]


def quotients(a, b):
    with mp.workdps(DPS + 10):
        return [_mpf(p) / _mpf(q) for p, q in zip(a, b)]


def errors(got, ref):
    """|got_i - ref_i| as float64 (got: floats or Fractions that a float holds exactly)."""
    with mp.workdps(DPS + 10):
        return np.array([float(abs(_mpf(g) - r)) for g, r in zip(got, ref)])


def trig_scale(xs, ref, F, pair):
    """scale_i of the trig kernels (see the module text)."""
    K = sincos_constants(F) if pair else sin_constants(F)
    P = float(K["hi"])
    half_ulp_lo = 0.5 * float(ulp(float(K["lo"]), F))
    x = np.array([float(v) for v in xs])
    return ulp(np.array([float(r) for r in ref]), F) + np.abs(x) / P * half_ulp_lo


def sinh_big_bound(xs, F):
    """First-order running error bound of sinh_pos's exponential form (e - 1 / e) / 2, e = exp(x) from a library good to one
    ulp: ulp_T(e) on e, that error carried through the quotient (ulp_T(e) / e^2) plus the quotient's own rounding (u / e), the
    rounding of the difference (u (e - 1 / e)); the halving is exact.  u = 2^-p."""
    u = 2.0 ** -F.p
    with mp.workdps(DPS):
        e = np.array([float(mp.exp(_mpf(x))) for x in xs])
    ue = ulp(e, F)
    return 0.5 * (ue + ue / e ** 2 + u / e + u * (e - 1 / e))


def plain_scale(ref, F):
    return ulp(np.array([float(r) for r in ref]), F)


def ratios(got, ref, scale):
    return errors(got, ref) / scale


# ---- input tables ------------------------------------------------------------------------------------------------------
def _as(F, v):
    return np.asarray(v, dtype=np.float64).astype(F.np).astype(np.float64)


def _neighbours(F, v):
    v = np.asarray(v, dtype=np.float64).astype(F.np)
    out = np.concatenate([np.nextafter(v, F.np(-np.inf)), v, np.nextafter(v, F.np(np.inf))])
    return np.concatenate([out, -out]).astype(np.float64)


@lru_cache(maxsize=None)
def trig_tables(fmt):
    """name -> float64 array of T-representable inputs, all inside the fast-path limit.  fp32's limit is 32768, so its two
    wide tables are +-1e4 and [1e4, limit) where fp64 has +-1e6 and [1e6, limit)."""
    F = FMT[fmt]
    rng = np.random.default_rng(20260 + F.p)
    n = 1024
    wide = 1e6 if F is F64 else 1e4
    t = {
        "pm_pio2": _as(F, rng.uniform(-np.pi / 2, np.pi / 2, n)),
        "pm_100": _as(F, rng.uniform(-100, 100, n)),
        "pm_wide": _as(F, rng.uniform(-wide, wide, n)),
        "to_limit": _as(F, rng.uniform(wide, F.limit, n) * rng.choice([-1.0, 1.0], n)),
    }
    kmax = int(F.limit / (np.pi / 2)) - 1
    ks = list(range(1, 65))
    j = 0
    while 2 ** j + 1 <= kmax:
        ks += [2 ** j - 1, 2 ** j, 2 ** j + 1]
        j += 1
    ks = sorted(set(k for k in ks if k >= 1))
    ks_rand = sorted(set(int(k) for k in rng.integers(65, kmax, n)))
    with mp.workdps(DPS):
        small = [float(k * mp.pi / 2) for k in ks]
        rand = [float(k * mp.pi / 2) for k in ks_rand]
    t["near_kpio2"] = _neighbours(F, small)
    t["near_kpio2_random"] = _neighbours(F, rand)
    for name, v in t.items():
        assert np.all(np.abs(v) < F.limit) and np.array_equal(v, _as(F, v)), name
    assert {k % 4 for k in ks} == {0, 1, 2, 3} and {k % 4 for k in ks_rand} == {0, 1, 2, 3}
    return t


@lru_cache(maxsize=None)
def tiny_table(fmt):
    """|x| < 2^-27 down to the denormals, both signs: sin x == x and cos x == 1 exactly."""
    F = FMT[fmt]
    rng = np.random.default_rng(7 + F.p)
    lo = F.emin - (F.p - 1)
    e = rng.uniform(lo, -27, 500)
    v = _as(F, np.concatenate([2.0 ** e * rng.choice([-1.0, 1.0], 500), [2.0 ** lo, -2.0 ** lo, 2.0 ** F.emin, -2.0 ** F.emin,
                                                                         2.0 ** -27 * (1 - 2.0 ** -F.p), -2.0 ** -27 * (1 - 2.0 ** -F.p)]]))
    v = v[v != 0]
    assert np.all(np.abs(v) < 2.0 ** -27)
    return v


def last_fast(F):
    """The last value of the fast path: limit - 1 ulp."""
    return float(np.nextafter(F.np(F.limit), F.np(0)))


@lru_cache(maxsize=None)
def poly_tables(fmt):
    """Inputs of the polynomial functions: name -> float64 array of T-representable values."""
    F = FMT[fmt]
    rng = np.random.default_rng(99 + F.p)
    eps = 2.0 ** -F.p
    den = 2.0 ** (F.emin - (F.p - 1))

    def sym(bound, n=768, nlog=256):
        e = rng.uniform(F.emin - (F.p - 1), np.log2(bound), nlog)
        edge = bound * (1 - eps)
        v = np.concatenate([rng.uniform(-bound, bound, n), 2.0 ** e * rng.choice([-1.0, 1.0], nlog),
                            [edge, -edge, den, -den, 2.0 ** F.emin, -2.0 ** F.emin, 0.0]])
        v = _as(F, v)
        return v[np.abs(v) < bound]
    x = _as(F, np.concatenate([rng.uniform(0, 0.5, 768), 2.0 ** rng.uniform(-40, -1, 256), [0.0, 0.5 * (1 - eps), 2.0 ** -20]]))
    x = x[x < 0.5]
    x2 = _as(F, x * x) if F is F64 else (x.astype(np.float32) * x.astype(np.float32)).astype(np.float64)
    big = _as(F, np.concatenate([rng.uniform(0.5, 40, 768), [0.5, float(np.nextafter(F.np(0.5), F.np(1))), 1.0, 40.0]]))
    return {"exp_inc": sym(2.0 ** -5), "exp_inc_tiny": sym(2.0 ** -15), "series_x2": x2[x2 < 0.25], "sinh_small": x, "sinh_big": big}


# ---- what is measured where ---------------------------------------------------------------------------------------------
# key -> (model, constants, reference name, which result of the model, trig pair?, table names)
def _trig_inputs(fmt):
    return np.concatenate(list(trig_tables(fmt).values()))


POLY = {
    "sin": (model_sin, sin_constants, "sin", None, False),
    "sincos_s": (model_sincos, sincos_constants, "sin", 0, True),
    "sincos_c": (model_sincos, sincos_constants, "cos", 1, True),
    "exp_inc": (model_exp_inc, exp_inc_constants, "exp", None, None),
    "exp_inc_tiny": (model_exp_inc_tiny, exp_inc_tiny_constants, "exp", None, None),
    "sinhc": (model_sinhc, lambda F: series_constants(SINHC_DEN, F), "sinhc", None, None),
    "coshc": (model_coshc, lambda F: series_constants(COSHC_DEN, F), "coshc", None, None),
    "sinh_small": (model_sinh_small, lambda F: series_constants(SINHC_DEN, F), "sinh", None, None),
}


# where the source leaves a * b + c to the compiler: measured at both contraction extremes
AMBIGUOUS = {("sincos_s", "f64"), ("sincos_c", "f64")} | {(k, f) for k in ("sinhc", "coshc", "sinh_small") for f in ("f64", "f32")}


def trig_slices(fmt):
    """table name -> slice of inputs_of(<trig key>, fmt)"""
    out, at = {}, 0
    for name, v in trig_tables(fmt).items():
        out[name] = slice(at, at + len(v)); at += len(v)
    return out


def inputs_of(key, fmt):
    if key in ("sin", "sincos_s", "sincos_c"):
        return _trig_inputs(fmt)
    return poly_tables(fmt)[{"sinhc": "series_x2", "coshc": "series_x2"}.get(key, key)]


@lru_cache(maxsize=None)
def reference_of(key, fmt):
    """(mpf references, scale) of POLY[key] over inputs_of(key, fmt): built once, shared by every test."""
    F = FMT[fmt]
    _, _, refname, _, pair = POLY[key]
    xs = inputs_of(key, fmt)
    ref = refs(refname, xs)
    scale = plain_scale(ref, F) if pair is None else trig_scale(xs, ref, F, pair)
    return ref, scale


@lru_cache(maxsize=None)
def _model_outputs(model, fmt, fused, series):
    xs = poly_tables(fmt)["series_x2"] if series else inputs_of({model_sin: "sin", model_sincos: "sincos_s", model_exp_inc: "exp_inc",
                                                                 model_exp_inc_tiny: "exp_inc_tiny", model_sinh_small: "sinh_small"}[model], fmt)
    return [model(Fraction(float(x)), FMT[fmt], None, fused) for x in xs]


def model_ratio(key, fmt, K=None, idx=None):
    """Largest error / scale of the restatement over inputs_of(key, fmt) (idx: a subset), over both contraction extremes."""
    F = FMT[fmt]
    model, _, _, which, _ = POLY[key]
    xs = inputs_of(key, fmt)
    ref, scale = reference_of(key, fmt)
    idx = range(len(xs)) if idx is None else idx
    worst = 0.0
    for fused in ((True, False) if (key, fmt) in AMBIGUOUS else (True,)):
        if K is None and isinstance(idx, range) and len(idx) == len(xs):
            out = _model_outputs(model, fmt, fused, key in ("sinhc", "coshc"))      # (the pair's two results share one pass)
        else:
            out = [model(Fraction(float(xs[i])), F, K, fused) for i in idx]
        got = [v if which is None else v[which] for v in out]
        e = errors(got, [ref[i] for i in idx])
        worst = max(worst, float(np.max(e / scale[list(idx)])))
    return worst


# Largest error / scale of the restatement on the tests' inputs (model_ratio; re-measured by the host test).  M = this + 1.
MODEL_MAX = {
    ("sin", "f64"): 2.019, ("sincos_s", "f64"): 1.231, ("sincos_c", "f64"): 1.268, ("exp_inc", "f64"): 0.639,
    ("exp_inc_tiny", "f64"): 0.499, ("sinhc", "f64"): 1.904, ("coshc", "f64"): 1.379, ("sinh_small", "f64"): 1.234,
    ("sin", "f32"): 1.862, ("sincos_s", "f32"): 1.379, ("sincos_c", "f32"): 1.350, ("exp_inc", "f32"): 0.503,
    ("exp_inc_tiny", "f32"): 0.500, ("sinhc", "f32"): 1.895, ("coshc", "f32"): 1.415, ("sinh_small", "f32"): 1.356,
}
# Bounds of the functions seeded by a hardware estimate, in ulp of the exact result (device_math.h's own statements).
HW_BOUND = {("RCP", "f64"): 1.0, ("DIVQ", "f64"): 1.0, ("DIVX", "f64"): 1.0, ("DIV", "f64"): 1.0, ("SQRTQ", "f64"): 1.0,
            ("SQRT", "f32"): 1.0, ("DIV", "f32"): 2.0}
LIBRARY_ULP = 4.0              # lanes at or above the limit: the OpenCL bound of the device library's sin / cos


def perturbation_subset(key, fmt):
    """The inputs the sensitivity check evaluates: every 8th of the trig tables, all of a polynomial's."""
    n = len(inputs_of(key, fmt))
    return range(0, n, 8) if POLY[key][4] is not None else range(n)


def M(key, fmt):
    return MODEL_MAX[(key, fmt)] + 1.0


# ---- perturbations -------------------------------------------------------------------------------------------------------
def perturbations(key, fmt):
    """name -> (constants with one entry changed, by `size`): every polynomial coefficient by 1e-3 relative, *_hi by one ulp,
    *_lo by 2^-20 relative.  Returns a function size_factor -> {name: K}; size_factor 1 is the sizes just named."""
    F = FMT[fmt]
    base = POLY[key][1](F)

    def make(f):
        out = {}
        if isinstance(base, dict):
            for name, v in base.items():
                if name == "inv":
                    continue
                if name == "hi":
                    K = dict(base); K["hi"] = v + Fraction(float(ulp(float(v), F))) * f; out["hi"] = K
                elif name == "lo":
                    K = dict(base); K["lo"] = rnd(v * (1 + Fraction(f, 2 ** 20)), F); out["lo"] = K
                else:
                    for i, cf in enumerate(v):
                        K = dict(base); K[name] = list(v); K[name][i] = rnd(cf * (1 + Fraction(f, 1000)), F); out["%s%d" % (name, i)] = K
        else:
            for i, cf in enumerate(base):
                K = list(base); K[i] = rnd(cf * (1 + Fraction(f, 1000)), F); out["c%d" % i] = K
        return out
    return make


# Perturbations the tests' inputs cannot see at the nominal size, with the factor (a power of 4 times the nominal size) at
# which they are seen; None: not seen up to 4^14 times the nominal size.  All of them are the highest terms of a polynomial
# or series, which lie below the last place of the result over the whole domain (the series carry fp64's eight terms in
# fp32 too; exp_increment's last term is 5e-18 relative at |d| = 2^-5): no test of values can see them, and none needs to.
UNDETECTED = {
    ("exp_inc", "f64", "c0"): 64, ("exp_inc_tiny", "f64", "c0"): 64,
    ("sinhc", "f64", "c6"): 1024, ("sinhc", "f64", "c7"): 1048576,
    ("coshc", "f64", "c6"): 64, ("coshc", "f64", "c7"): 65536,
    ("sinh_small", "f64", "c5"): 16, ("sinh_small", "f64", "c6"): 16384, ("sinh_small", "f64", "c7"): 16777216,
    ("sincos_s", "f32", "S2"): 4, ("sincos_s", "f32", "S3"): 1024, ("sincos_s", "f32", "C2"): 64,
    ("sincos_c", "f32", "S2"): 4, ("sincos_c", "f32", "S3"): 1024, ("sincos_c", "f32", "C2"): 64,
    ("exp_inc", "f32", "c0"): 4096, ("exp_inc", "f32", "c1"): 16, ("exp_inc_tiny", "f32", "c0"): 262144,
    ("sinhc", "f32", "c2"): 4, ("sinhc", "f32", "c3"): 1024, ("sinhc", "f32", "c4"): 1048576, ("sinhc", "f32", "c5"): 268435456,
    ("sinhc", "f32", "c6"): None, ("sinhc", "f32", "c7"): None,
    ("coshc", "f32", "c3"): 256, ("coshc", "f32", "c4"): 65536, ("coshc", "f32", "c5"): 67108864,
    ("coshc", "f32", "c6"): None, ("coshc", "f32", "c7"): None,
    ("sinh_small", "f32", "c2"): 64, ("sinh_small", "f32", "c3"): 16384, ("sinh_small", "f32", "c4"): 16777216,
    ("sinh_small", "f32", "c5"): None, ("sinh_small", "f32", "c6"): None, ("sinh_small", "f32", "c7"): None,
}
