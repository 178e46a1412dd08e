"""Every opcode of a loaded expression (include/rovmpc.h, rovmpc_opcode) against 50-digit mpmath: the evaluator, its running
error bound, the input tables and the composite expressions of tests/test_expr_paths_gpu.py.

The law.  An expression is evaluated in T (float64 or float32) operation by operation, in Python's evaluation order, on slots
that T holds exactly.  Constants are rounded to T once (interp_eval reads them from a T array, the hiprtc text has T(...)
literals); safe_log(x) = log(|x| + T(1e-5)), safe_sqrt(x) = sqrt(|x|); x**2 is a square, x**e with an integer-valued literal
|e| < 2^22 is square-and-multiply (reciprocal last for e < 0), every other power is pow.  The evaluator below walks the TEXT
with Python's `ast` -- it shares nothing with the product's compiler -- and returns the exact value of the expression on the
given slots together with an error scale.

Error scale.  A first-order running bound: an operation with exact result v adds c_op * u_T * |v| (u_T = 2^(1-p), never less
than c_op times T's smallest subnormal) and passes its operands' bounds on through |df/d operand|.
  c_op = 1/2   + - * abs neg square: correctly rounded (derived)
  POWI         (|e| - 1) / 2 for square-and-multiply, + 1/2 for the reciprocal of e < 0 (derived: powi_roundings)
  /  sin  cos  DESIGN.md section 3: m_divx 1; m_sin / Trig::sin 3.02 (fp64) 2.86 (fp32); m_cos 2.27 / 2.35.  The trig bounds
               are in the unit of that table, u |v| + (|x| / P) * 1/2 ulp(P_lo), P = pi (sine) or pi/2 (cosine)
  tanh exp log sqrt pow   NP_MODEL + 1: NP_MODEL is NumPy's own largest error over this module's regular tables (float64
               ufuncs, and float32 ufuncs for the fp32 law), measured against mpmath in u |v|, rounded up to two places;
               tests/test_expr_reference_host.py measures it again.  The ROCm install documents no bound for the device
               library's functions, so none replaces these.
A result is within bound when |got - exact| <= scale; where NumPy's value is NaN, +-inf or +-0 the result must be that value,
sign included.  Values come from NumPy (oracle.SymbolicModel), generated when the tables are built, never typed in.

Stated deviations (include/rovmpc.h), pinned here: sin(-0.0) = +0.0; x**e with e < 0 is 1 / x**|e|, so where x**|e|
overflows the result is a zero where NumPy keeps a subnormal; fp32 only, sqrt reads a subnormal operand as a zero of its sign
(v_sqrt_f32), so sqrt(1e-45) = 0 and sqrt(-1e-45) = -0 where NumPy gives 3.7e-23 and NaN; hiprtc route only, a / D with a
stage-invariant D is a * (1 / D), pinned by tests/test_expr_paths_gpu.py where 1 / D is not a normal number."""
import ast
from functools import lru_cache

import mpmath as mp
import numpy as np

import device_math_reference as dm

DPS = 50
MAX_STACK, MAX_CODE, MAX_SUBS, MAX_GSUBS = 16, 256, 8, 2
POWI_LIMIT = 1 << 22


class Fmt:
    def __init__(self, name, p, np_type):
        self.name, self.p, self.np = name, p, np_type
        self.eps = 2.0 ** (1 - p)
        self.tiny = float(np.finfo(np_type).smallest_subnormal)
        self.max = float(np.finfo(np_type).max)
        self.dm = dm.FMT[name]

    def __repr__(self):
        return self.name


F64, F32 = Fmt("f64", 53, np.float64), Fmt("f32", 24, np.float32)
FMT = {"f64": F64, "f32": F32}

C_ROUND = 0.5
C_DIV = {"f64": 1.0, "f32": 1.0}
C_SIN = {"f64": 3.02, "f32": 2.86}
C_COS = {"f64": 2.27, "f32": 2.35}
# NumPy's own largest error / (u |v|) over the regular tables below (measure_numpy); the bound is this + 1
NP_MODEL = {("tanh", "f64"): 0.66, ("exp", "f64"): 0.52, ("log", "f64"): 0.49, ("sqrt", "f64"): 0.50, ("pow", "f64"): 0.54,
            ("tanh", "f32"): 0.57, ("exp", "f32"): 1.23, ("log", "f32"): 1.17, ("sqrt", "f32"): 0.50, ("pow", "f32"): 0.86}


def c_lib(name, F):
    return NP_MODEL[(name, F.name)] + 1.0


@lru_cache(maxsize=None)
def _half_ulp_lo(F, pair):
    K = dm.sincos_constants(F.dm) if pair else dm.sin_constants(F.dm)
    return float(K["hi"]), 0.5 * float(dm.ulp(float(K["lo"]), F.dm))


# ---- the evaluator ---------------------------------------------------------------------------------------------------------
class _Undefined(Exception):
    """An operand or result outside the finite range of T, or outside a function's domain: NumPy's value decides."""


def powi_roundings(e):
    """Own error of square-and-multiply (interp_eval, rv_powi) in u |v|, first order.  With d the relative error of a factor
    in units of u: a square b <- b b has 2 d_b + 1/2, a product r <- r b has d_r + d_b + 1/2 (r = 1 * b is exact), the
    reciprocal of e < 0 adds 1/2.  That is (|e| - 1) / 2 (+ 1/2): the rounding of b^(2^j) enters the result once for every
    later use AND doubles with every later square, so a count of the multiplications alone is no bound (x**30: 7 products,
    yet IEEE arithmetic reaches 9.4 u at x = 0.526; this gives 14.5)."""
    ae, d_b, d_r, first = abs(e), 0.0, 0.0, True
    while ae:
        if ae & 1:
            d_r = d_b if first else d_r + d_b + C_ROUND
            first = False
        ae >>= 1
        if ae:
            d_b = 2 * d_b + C_ROUND                 # (the square after the last set bit is never used)
    return d_r + (C_ROUND if e < 0 else 0.0)


class Evaluator:
    def __init__(self, text, F):
        self.F = F
        self.tree = ast.parse(text.strip().replace("^", "**"), mode="eval").body

    def __call__(self, slots):
        """(exact value as mpf, error scale as float), or (None, None) when an operation leaves T's finite range or domain."""
        self.slots = slots
        try:
            with mp.workdps(DPS + 10):
                v, e = self._ev(self.tree)
            return v, e
        except _Undefined:
            return None, None

    @staticmethod
    def _thru(e, d):
        """An operand's bound e carried through |df/d operand| = d (an exact operand stays exact whatever d is)."""
        return e * float(abs(d)) if e else 0.0

    # own error of an operation with exact result v
    def _own(self, c, v):
        if not mp.isfinite(v):
            raise _Undefined
        a = abs(v)
        if a >= mp.mpf(self.F.max) * (1 + mp.mpf(self.F.eps) / 4):          # rounds to inf (max + 1/2 ulp and above)
            raise _Undefined
        return c * max(self.F.eps * float(a), self.F.tiny)

    @staticmethod
    def _number(node):
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)) and not isinstance(node.value, bool):
            return float(node.value)
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            v = Evaluator._number(node.operand)
            if v is not None:
                return -v if isinstance(node.op, ast.USub) else v
        return None

    def _leaf(self, x):
        x = float(self.F.np(x))
        if np.isnan(x):
            raise _Undefined
        return mp.mpf(x), 0.0                          # +-inf goes on as mpmath's: 1 / inf**|e| and a / inf are exact zeros, the rest ends in _own

    def _ev(self, node):
        F = self.F
        num = self._number(node)
        if num is not None:
            return self._leaf(num)
        if isinstance(node, ast.Name):
            return self._leaf(self.slots[int(node.id[1:])])
        if isinstance(node, ast.UnaryOp):
            v, e = self._ev(node.operand)
            if isinstance(node.op, ast.UAdd):
                return v, e
            return -v, e + self._own(C_ROUND, v)
        if isinstance(node, ast.BinOp):
            if isinstance(node.op, ast.Pow):
                ex = self._number(node.right)
                if ex is not None and ex == 2.0:
                    return self._call("square", [self._ev(node.left)])
                if ex is not None and float(ex).is_integer() and abs(ex) < POWI_LIMIT:
                    return self._powi(self._ev(node.left), int(ex))
                return self._call("pow", [self._ev(node.left), self._ev(node.right)])
            (a, ea), (b, eb) = self._ev(node.left), self._ev(node.right)
            if isinstance(node.op, ast.Add):
                v = a + b
                return v, ea + eb + self._own(C_ROUND, v)
            if isinstance(node.op, ast.Sub):
                v = a - b
                return v, ea + eb + self._own(C_ROUND, v)
            if isinstance(node.op, ast.Mult):
                v = a * b
                return v, self._thru(ea, b) + self._thru(eb, a) + self._own(C_ROUND, v)
            if isinstance(node.op, ast.Div):
                if b == 0:
                    raise _Undefined
                v = a / b
                return v, self._thru(ea, 1 / b) + self._thru(eb, v / b) + self._own(C_DIV[F.name], v)
            raise ValueError("operator")
        if isinstance(node, ast.Call):
            return self._call(node.func.id, [self._ev(a) for a in node.args])
        raise ValueError(ast.dump(node))

    def _powi(self, be, e):
        b, eb = be
        if e == 0:
            return mp.mpf(1), 0.0
        if mp.isinf(b):
            if e < 0:
                return mp.mpf(0), 0.0                   # 1 / inf: an exact zero (NumPy's value carries the sign)
            raise _Undefined
        if b == 0:
            if e > 0 and not eb:
                return mp.mpf(0), 0.0                   # an exact zero to a positive power: zero (NumPy's value carries the sign)
            raise _Undefined
        # an intermediate power that leaves the range decides the result on the device: NumPy's value is the judge there
        ae, sq = abs(e), b
        while ae > 1:
            sq = sq * sq
            ae >>= 1
            if abs(sq) > self.F.max or abs(sq) < self.F.tiny:
                raise _Undefined
        p = b ** abs(e)
        if abs(p) > self.F.max or abs(p) < self.F.tiny:
            raise _Undefined
        v = 1 / p if e < 0 else p
        own = self._own(powi_roundings(e), v)
        if e < 0:                                   # a subnormal b**|e| is rounded at T's smallest subnormal, not at u |p|
            own += float(powi_roundings(e) * mp.mpf(self.F.tiny) * abs(v / p))
        return v, self._thru(eb, e * v / b) + own

    def _call(self, fn, args):
        F = self.F
        if any(mp.isinf(a) for a, _ in args):
            raise _Undefined
        if fn in ("pow", "Pow"):
            (a, ea), (y, ey) = args
            if a == 0 and y > 0 and not ea:
                return mp.mpf(0), 0.0                   # pow(+-0, y > 0): an exact zero (NumPy's value carries the sign)
            if a == 0 or (a < 0 and (y != mp.floor(y) or ey)):
                raise _Undefined
            v = mp.power(a, y) if a > 0 else mp.power(-a, y) * (-1 if int(y) % 2 else 1)      # negative base, integer-valued exponent
            return v, self._thru(ea, y * v / a) + self._thru(ey, v * mp.log(abs(a))) + self._own(c_lib("pow", F), v)
        (x, ex), = args
        if fn in ("abs", "Abs"):
            return abs(x), ex + self._own(C_ROUND, x)
        if fn == "neg":
            return -x, ex + self._own(C_ROUND, x)
        if fn == "square":
            v = x * x
            return v, self._thru(ex, 2 * x) + self._own(C_ROUND, v)
        if fn == "sin":
            P, hl = _half_ulp_lo(F, False)
            v = mp.sin(x)
            return v, self._thru(ex, mp.cos(x)) + self._own(C_SIN[F.name], v) + C_SIN[F.name] * float(abs(x)) / P * hl
        if fn == "cos":
            P, hl = _half_ulp_lo(F, True)
            v = mp.cos(x)
            return v, self._thru(ex, mp.sin(x)) + self._own(C_COS[F.name], v) + C_COS[F.name] * float(abs(x)) / P * hl
        if fn == "tanh":
            v = mp.tanh(x)
            return v, self._thru(ex, 1 - v * v) + self._own(c_lib("tanh", F), v)
        if fn == "exp":
            v = mp.exp(x)
            return v, self._thru(ex, v) + self._own(c_lib("exp", F), v)
        if fn == "safe_log":
            x = abs(x) + mp.mpf(float(F.np(1e-5)))
            ex = ex + self._own(C_ROUND, x)
            fn = "log"
        if fn == "log":
            if x <= 0:
                raise _Undefined
            v = mp.log(x)
            return v, self._thru(ex, 1 / x) + self._own(c_lib("log", F), v)
        if fn == "safe_sqrt":
            x, fn = abs(x), "sqrt"
        if fn == "sqrt":
            if x < 0:
                raise _Undefined
            if x == 0:
                if ex:
                    raise _Undefined
                return mp.mpf(0), 0.0
            v = mp.sqrt(x)
            return v, self._thru(ex, 1 / (2 * v)) + self._own(c_lib("sqrt", F), v)
        raise ValueError(fn)


def numpy_values(text, X, F):
    """What NumPy gives: the oracle's evaluation of the text on the columns of X in T."""
    from oracle import rovmpc_oracle as orc
    X = np.asarray(X, dtype=np.float64).astype(F.np)
    ns_text = text.strip().replace("^", "**")
    with np.errstate(all="ignore"):
        out = orc.SymbolicModel(ns_text)([X[:, i] for i in range(X.shape[1])])
    return np.broadcast_to(np.asarray(out, dtype=F.np), (X.shape[0],)).astype(np.float64)


class Case:
    """One expression on a table of slot rows X (n, 18): NumPy's values, the exact values and the error scale."""

    def __init__(self, op, name, text, X, fmt, pinned=None):
        self.op, self.name, self.text, self.fmt = op, name, text, fmt
        F = FMT[fmt]
        self.X = np.asarray(X, dtype=np.float64).astype(F.np).astype(np.float64)
        self.numpy = numpy_values(text, self.X, F)          # NumPy's own values; `want` differs on the pinned rows alone
        self.want = self.numpy.copy()
        self.pinned = sorted(pinned or {})
        for i, v in (pinned or {}).items():
            self.want[i] = v                                # a stated deviation (module text)
        ev = Evaluator(text, F)
        refs = [ev(row) if i not in self.pinned else (None, None) for i, row in enumerate(self.X)]      # a pinned value is exact
        self.ref, self.scale = zip(*refs) if refs else ((), ())

    def ratios(self, got, extra=0.0):
        """error / (scale + extra) per row; 0 where a special value is matched exactly, inf where it is missed."""
        got = np.asarray(got, dtype=np.float64)
        out = np.zeros(len(got))
        with mp.workdps(DPS + 10):
            for i, (g, w, r, s) in enumerate(zip(got, self.want, self.ref, self.scale)):
                if np.isnan(w):
                    out[i] = 0.0 if np.isnan(g) else np.inf
                elif np.isinf(w) or (w == 0 and (r is None or r == 0)):
                    out[i] = 0.0 if (g == w and np.signbit(g) == np.signbit(w)) else np.inf
                elif r is None:
                    out[i] = 0.0 if (g == w or abs(g - w) <= extra) else np.inf   # finite behind a non-finite operand (pow(x, 0), tanh(inf)), or pinned: exact
                elif not np.isfinite(g):
                    out[i] = np.inf
                else:
                    out[i] = float(abs(mp.mpf(float(g)) - r)) / (s + extra) if s + extra > 0 else (0.0 if mp.mpf(float(g)) == r else np.inf)
        return out


# ---- tables ------------------------------------------------------------------------------------------------------------------
NREG = 256


def _rows(F, **cols):
    n = max(len(np.atleast_1d(v)) for v in cols.values())
    X = np.zeros((n, 18))
    for k, v in cols.items():
        X[:, int(k[1:])] = v
    return X.astype(F.np).astype(np.float64)


def _logspread(rng, n, lo, hi, signed=True):
    v = 2.0 ** rng.uniform(lo, hi, n)
    return v * rng.choice([-1.0, 1.0], n) if signed else v


@lru_cache(maxsize=None)
def regular_cases(fmt):
    """One Case per (opcode, form) on a few hundred points: spread over the range where the result is finite, dense at the
    cut-overs."""
    F = FMT[fmt]
    rng = np.random.default_rng(4100 + F.p)
    n, h = NREG, NREG // 2
    E = 300 if F is F64 else 30                         # exponent spread of the arithmetic tables
    xmax = 700.0 if F is F64 else 85.0
    sat = 19.0 if F is F64 else 9.0
    a, b = _logspread(rng, n, -E, E), _logspread(rng, n, -E, E)
    near = np.concatenate([_logspread(rng, h, -8, 8), rng.uniform(-4, 4, n - h)])
    c = near * (1 + rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-F.p, -1, n))          # a - c cancels
    trig = np.concatenate([rng.uniform(-100, 100, h), rng.uniform(-1e4, 1e4, 64),
                           (rng.integers(-40, 40, 64) * (np.pi / 2)) * (1 + 2.0 ** -rng.integers(10, F.p, 64))])
    th = np.concatenate([_logspread(rng, 64, -60 if F is F64 else -30, -1), rng.uniform(-3, 3, 64), rng.uniform(-sat, sat, 64),
                         rng.uniform(sat - 3, sat, 64) * rng.choice([-1.0, 1.0], 64)])
    ex = np.concatenate([rng.uniform(-xmax, xmax, h), _logspread(rng, 64, -60 if F is F64 else -30, 0), rng.uniform(-2, 2, 64)])
    pos = np.concatenate([_logspread(rng, h, -1000 if F is F64 else -120, 1000 if F is F64 else 120, False),
                          1 + rng.uniform(-1, 1, 64) * 2.0 ** rng.integers(-F.p + 1, -1, 64), rng.uniform(0.25, 4, 64)])
    pb = np.concatenate([_logspread(rng, h, -40, 40, False), 1 + rng.uniform(-1, 1, 64) * 2.0 ** rng.integers(-F.p + 1, -2, 64),
                         rng.uniform(0.25, 4, 64)])
    py = np.concatenate([rng.uniform(-6, 6, h), rng.uniform(-40, 40, 64), _logspread(rng, 64, -40 if F is F64 else -20, -2)])
    pw = rng.uniform(-3, 3, n) + _logspread(rng, n, -3, 3) * 0                        # bases of the integer powers
    pw = np.where(np.abs(pw) < 0.05, 0.7, pw)
    sl = np.concatenate([_logspread(rng, h, -60 if F is F64 else -40, 20), rng.uniform(-3e-5, 3e-5, 64), rng.uniform(-3, 3, 64)])
    R = lambda **k: _rows(F, **k)
    spec = [
        ("ADD", "x0 + x1", R(x0=a, x1=b)), ("ADD", "x0 + x1", R(x0=near, x1=-c)), ("SUB", "x0 - x1", R(x0=near, x1=c)),
        ("SUB", "x0 - x1", R(x0=a, x1=b)), ("MUL", "x0 * x1", R(x0=_logspread(rng, n, -E / 2, E / 2), x1=_logspread(rng, n, -E / 2, E / 2))),
        ("DIV", "x0 / x1", R(x0=_logspread(rng, n, -E / 2, E / 2), x1=_logspread(rng, n, -E / 2, E / 2))),
        ("NEG", "-(x0 + x1)", R(x0=near, x1=-c)), ("NEG", "neg(x0 * x1)", R(x0=near, x1=c)), ("ABS", "abs(x0 - x1)", R(x0=near, x1=c)),
        ("ABS", "Abs(x0)", R(x0=a)), ("SQUARE", "square(x0)", R(x0=_logspread(rng, n, -E / 2, E / 2))),
        ("SQUARE", "x0**2", R(x0=near)), ("SIN", "sin(x0)", R(x0=trig)), ("COS", "cos(x0)", R(x0=trig)),
        ("TANH", "tanh(x0)", R(x0=th)), ("EXP", "exp(x0)", R(x0=ex)), ("LOG", "log(x0)", R(x0=pos)), ("SQRT", "sqrt(x0)", R(x0=pos)),
        ("POW", "x0**x1", R(x0=pb, x1=py)), ("POW", "pow(x0, x1)", R(x0=pb, x1=py[::-1])), ("POW", "x0**2.5", R(x0=pb)),
        ("POW", "x0^-0.5", R(x0=pb)), ("POW", "1.5**x0", R(x0=py)),
        ("SAFE_LOG", "safe_log(x0)", R(x0=sl)), ("SAFE_SQRT", "safe_sqrt(x0)", R(x0=a)),
        ("PUSH_C", "x0 * 0.1 + 1.0000000000000002", R(x0=near)), ("PUSH_F", "x17 - x3", R(x17=near, x3=c)),
    ]
    for e in (3, 5, 30, -1, -2, -3, -7):
        spec.append(("POWI", "x0**%d" % e if e > 0 else "x0**(%d)" % e, R(x0=pw)))
    return [Case(op, "%s[%d]" % (op, i), text, X, fmt) for i, (op, text, X) in enumerate(spec)]


LIB_OPS = {"tanh": "TANH", "exp": "EXP", "log": "LOG", "sqrt": "SQRT", "pow": "POW"}


def measure_numpy(fmt):
    """NumPy's largest error / (u |v|) per library function over the regular tables: what NP_MODEL records."""
    F = FMT[fmt]
    out = {}
    with mp.workdps(DPS + 10):
        for fn, op in LIB_OPS.items():
            worst = 0.0
            for case in regular_cases(fmt):
                if case.op != op:
                    continue
                for g, r in zip(case.want, case.ref):
                    if r is not None and np.isfinite(g):
                        worst = max(worst, float(abs(mp.mpf(float(g)) - r)) / max(F.eps * float(abs(r)), F.tiny))
            out[fn] = worst
    return out


def stated_pins(op, operand, F, e=None):
    """index -> value on the rows where a stated deviation (module text) replaces NumPy's value.  `operand`: the column the
    opcode reads; e: the exponent of a POWI."""
    x = np.asarray(operand, dtype=np.float64).astype(F.np)
    if op == "POWI" and e is not None and e < 0:
        with np.errstate(all="ignore"):
            p = (x ** F.np(abs(e))).astype(np.float64)
        return {i: float(np.copysign(0.0, p[i])) for i in range(len(x)) if np.isinf(p[i])}
    if op in ("SQRT", "SAFE_SQRT") and F is F32:
        tiny = np.finfo(np.float32).tiny
        return {i: float(np.copysign(0.0, x[i])) if op == "SQRT" else 0.0 for i in range(len(x)) if x[i] != 0 and abs(x[i]) < tiny}
    return {}


def _special_values(F):
    t = np.finfo(F.np)
    return dict(den=float(t.smallest_subnormal), mn=float(t.tiny), mx=float(t.max), big=float(t.max) / 2 * 1.5)


@lru_cache(maxsize=None)
def special_cases(fmt):
    """Special operands per opcode; the expected values are NumPy's, generated here."""
    F = FMT[fmt]
    s = _special_values(F)
    den, mn, mx, big = s["den"], s["mn"], s["mx"], s["big"]
    inf, nan = np.inf, np.nan
    R = lambda **k: _rows(F, **k)
    lmx = float(np.log(F.np(mx)))
    lo_edge = float(np.log(F.np(den)))
    cases = []
    add = lambda op, text, X, pinned=None: cases.append(Case(op, "%s*[%d]" % (op, len(cases)), text, X, fmt, pinned))
    add("LOG", "log(x0)", R(x0=[0.0, -0.0, -1.0, -den, inf, -inf, nan, den, mn, 1.0, mx]))
    sq = [0.0, -0.0, -1.0, -den, inf, -inf, nan, den, 3 * den, mn / 2, mn, mx, 4.0]
    add("SQRT", "sqrt(x0)", R(x0=sq), pinned=stated_pins("SQRT", sq, F))
    add("SAFE_SQRT", "safe_sqrt(x0)", R(x0=sq), pinned=stated_pins("SAFE_SQRT", sq, F))
    add("SAFE_LOG", "safe_log(x0)", R(x0=[0.0, -0.0, inf, -inf, nan, den, -den, -1.0, mx]))
    e_in = [lmx, np.nextafter(F.np(lmx), F.np(inf)), lmx + 1, 1000.0, lo_edge, lo_edge - 1, np.nextafter(F.np(lo_edge), F.np(-inf)),
            -1000.0, inf, -inf, nan, 0.0, -0.0, den]
    add("EXP", "exp(x0)", R(x0=e_in))
    add("TANH", "tanh(x0)", R(x0=[inf, -inf, 0.0, -0.0, nan, 20.0, -20.0, 25.0, 1000.0, -1000.0, den, -den, mx]))
    z = [0.0, -0.0, nan, inf, -inf, 1.0, -den]
    add("ABS", "abs(x0)", R(x0=z)); add("NEG", "-x0", R(x0=z)); add("NEG", "neg(x0)", R(x0=z))
    add("SIN", "sin(x0)", R(x0=[-0.0, 0.0, den, -den, nan]), pinned={0: 0.0})
    add("COS", "cos(x0)", R(x0=[-0.0, 0.0, den, nan]))
    # pow, C99 Annex F
    pb = [2.0, -2.0, nan, inf, 0.0, nan, 1.0, 1.0, 1.0, -2.0, -8.0, -2.0, -2.0, -2.0, -2.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0,
          inf, -inf, inf, -inf, -inf, -inf, -inf, 0.5, 2.0, 0.5, 2.0, -1.0, -1.0, nan, 2.0, den, mx, mx, 0.0, -0.0]
    py = [0.0, -0.0, 0.0, 0.0, 0.0, -0.0, nan, inf, -inf, 0.5, 1.0 / 3, 3.0, 4.0, -3.0, -4.0, -3.0, -3.0, -4.0, -4.0, 3.0, 3.0, 4.0, 4.0,
          2.5, 3.0, -2.5, -3.0, 4.0, 2.5, -4.0, inf, inf, -inf, -inf, inf, -inf, 1.0, nan, 0.5, 2.0, 0.5, 0.5, 0.5]
    add("POW", "x0**x1", R(x0=pb, x1=py))
    add("POW", "pow(x0, x1)", R(x0=pb, x1=py))
    add("POW", "x0**4194304.0", R(x0=[1.0, -1.0, 0.0, -0.0, inf, -inf, nan, 1 + F.eps, 0.5, 2.0]))      # 2^22: falls through to POW
    add("POW", "x0**-4194304", R(x0=[1.0, -1.0, 0.0, -0.0, inf, -inf, nan, 1 + F.eps, 0.5, 2.0]))
    base = [0.0, -0.0, 1.0, -1.0, nan, inf, -inf]
    for e in (0, 1, 3, 5, 30, -1, -2, -3, -7, POWI_LIMIT - 1, -(POWI_LIMIT - 1)):
        add("POWI", "x0**(%d)" % e, R(x0=base))
    # bases where an intermediate square overflows or underflows
    rt = float(np.sqrt(F.np(mx))); rs = float(np.sqrt(F.np(mn)))
    edge = [rt * 1.01, -rt * 1.01, rt * 0.99, rs * 0.99, -rs * 0.99, rs * 1.01, float(F.np(mx) ** F.np(0.25)) * 1.5, mx, mn, den, -den,
            float(F.np(mx) ** F.np(1 / 7.0)) * 1.01, float(F.np(mx) ** F.np(1 / 7.0)) * 0.99, float(F.np(mn) ** F.np(1 / 3.0)) * 0.9]
    for e in (3, 5, 30, -2, -3, -7):
        c = Case("POWI", "", "x0**(%d)" % e, R(x0=edge), fmt, pinned=stated_pins("POWI", edge, F, e))
        c.name = "POWI*[%d]" % len(cases)
        cases.append(c)
    return cases


@lru_cache(maxsize=None)
def division_cases(fmt):
    """a / D at extreme divisors: the table of the reciprocal rewrite of the code generator (D in x3: stage-invariant; a in
    x15: the stage's gamma)."""
    F = FMT[fmt]
    s = _special_values(F)
    den, mn, mx, big = s["den"], s["mn"], s["mx"], s["big"]
    D = [den, -den, 37 * den, mn, 2 * mn, -mn, 1 / mn, -1 / mn, 2 / mn, mx / 2 * 1.0000001, big, -big, mx, 0.0, -0.0, np.inf, -np.inf, np.nan, mn / 4, 3.0, -7.0]
    A = [1.0, -3.0, mn * 3, den * 5, mx / 3, 0.0, 1e-3 if F is F32 else 1e-300]
    dd, aa = np.meshgrid(D, A)
    rng = np.random.default_rng(77 + F.p)
    E = 200 if F is F64 else 20
    dd = np.concatenate([dd.ravel(), _logspread(rng, 64, -E, E)]); aa = np.concatenate([aa.ravel(), _logspread(rng, 64, -E, E)])
    return Case("DIV", "DIV/extreme", "x15 / x3", _rows(F, x3=dd, x15=aa), fmt)


# ---- composite expressions for the code generator (generation-1 map: x0..x13 exogenous, x14 / x15 the stage's state, x16 /
# x17 the delay slots; state_mask of jit_source = x14..x17, gmask = x17) -------------------------------------------------------
HEAVY = {
    "exp": "exp(%s)", "log": "log(%s)", "sqrt": "sqrt(%s)", "tanh": "tanh(%s)", "pow": "(%s)**1.5", "safe_log": "safe_log(%s)",
    "safe_sqrt": "safe_sqrt(%s)", "sin": "sin(%s)", "cos": "cos(%s)", "powi_neg": "(%s)**(-3)",
}


def composite_theta(op):
    """dtheta/dt row for one heavy opcode: (a) exogenous only -> e[k]; (b) x17 only -> g[k] under a candidate-invariant gamma
    row; (c) reads x15 -> stays in the stage; (d) a mixed product and quotient, where each side's class is lost; the (a)
    subtree a second time (one e[k]); a / D with D in each class."""
    H = lambda a: HEAVY[op] % a
    return " + ".join([H("x3 + x4"), H("x17 * 0.75"), H("x15 + x4"), "%s * %s / %s" % (H("x5"), H("x17 * 0.75"), H("x15")),
                       "x15 * %s" % H("x3 + x4"), "x15 / %s" % H("x6"), "x16 / (x17 + 1.25)", "x4 / (x15 + x16)"])


def composite_gamma(op):
    """dgamma/dt row on (x15, x17) alone: the gamma path stays candidate-invariant."""
    return "%s - x15 * 0.5" % (HEAVY[op] % "x17 + 0.5")


OVERFLOW_THETA = " + ".join(["x15 * exp(x%d * %r)" % (i, 0.1 * (i + 1)) for i in range(9)] + ["tanh(x17)", "sqrt(x17)", "log(x17 + 2.0)"])
# constants: 1e999 is how the text grammar spells inf (there is no literal for NaN: it is computed), -0.0, all 17 digits
CONSTANT_ROWS = ("x15 + -1e999", "x15 * (1e999 - 1e999)", "x3 * -0.0", "x4 / 1e999", "x15 - 1e999",
                 "x15 * 0.12345678901234568 + 0.30000000000000004")


def deep_expression(depth=MAX_STACK):
    """Right-nested sum that needs exactly `depth` stack slots."""
    names = ["x%d" % (i % 9) for i in range(depth)]
    text = names[-1]
    for nm in reversed(names[:-1]):
        text = "%s - (%s)" % (nm, text)
    return text


def long_expression(n_ins=MAX_CODE):
    """Left-nested chain of exactly n_ins instructions (n_ins even: one unary on top)."""
    k = (n_ins - (n_ins % 2 == 0)) // 2                     # 2 k + 1 instructions for k binary operations
    text = "x0"
    for i in range(k):
        text = "(%s %s x%d)" % (text, "+-"[i % 2], 1 + i % 8) if i % 5 else "(%s * %r)" % (text, 1.0 + 2.0 ** -(i % 40 + 1))
    return "abs(%s)" % text if n_ins % 2 == 0 else text


def all_texts():
    out = [c.text for f in ("f64",) for c in regular_cases(f) + special_cases(f)] + [division_cases("f64").text]
    out += [composite_theta(op) for op in HEAVY] + [composite_gamma(op) for op in HEAVY]
    out += [OVERFLOW_THETA, deep_expression(), long_expression()] + list(CONSTANT_ROWS)
    return list(dict.fromkeys(out))
