"""rovmpc_refit_rows (include/rovmpc.h) restated in NumPy and at 50 digits, the bound on what a converged fit may lose against
the exact minimiser, and the fixtures of tests/test_refit_reference_host.py and tests/test_refit_gpu.py.

refit_np    the law in NumPy: fp64, the law's tangent rules and summation order (TILE partial sums per lane, recording after
            recording, then the tree), its step, its stops.  The library functions are NumPy's, so its bits are not the device's.
refit_mp    the same law at 50 digits (mpmath forward mode over the bytecode), run to gtol = 1e-30 with xtol = 0: the exact
            minimiser c* that the start leads to, F* = F(c*), and what the bound needs there.
Both read the bytecode of the product's compiler; the tangent rules are written here a second time.

The bound (check 3 of the GPU test).  A fit that stopped on the orthogonality test has |g_j| <= gtol sqrt(A_jj F) for all j.
To first order (the Gauss-Newton model F(c + d) = F + 2 g.d + d.A d, minimised by d = -A^-1 g) it is above the minimum by
g.A^-1 g.  With D = diag(A)^(1/2), gs = D^-1 g and As = D^-1 A D^-1 (unit diagonal): g.A^-1 g = gs.As^-1 gs <= |gs|^2 / lmin(As)
<= P gtol^2 F / lmin.  The sum F itself is rounded: n + 2 roundings per term chain, gamma_{n+2} F (score_reference).  So
    F_got - F* <= F* (P gtol^2 / lmin + gamma_{n+2} + u) + VALUE
The same reasoning gives the distance of the constants: D (c - c*) = -As^-1 gs, so |c_j - c*_j| <= sqrt(P F) gtol / (lmin sqrt(A_jj)) + VALUE_j.
VALUE is what cannot be derived here: the values p_i carry the rounding of the row's operations, |eps_i| <= k u |p_i| with a k
that depends on the row (expr_reference derives it per operation), and a fit whose last steps are rejected because F no longer
decreases in fp64 stops on the step test at a point that the orthogonality test has not certified.  Both scale the same way:
a perturbation eps of the values changes F by at most 2 |r| |eps| + |eps|^2, i.e. E = 2 u |p| sqrt(F*) + u^2 |p|^2 with |p|^2 =
sum p_i^2, and moves the minimiser by A^-1 J^T eps, |D dc| <= |eps| / sqrt(lmin), i.e. E_j = u |p| / sqrt(lmin A_jj).  VALUE =
4 M E and VALUE_j = 4 M_c E_j with M, M_c the largest (F_np - F* - derived part) / E and (|c_np - c*| - derived part) / E_j of the
NumPy restatement (never the GPU), M over every converged problem of fixtures A and B, M_c over those of B (the constants are
asserted there alone: several fits of A stop on the step test with orth up to 1.4e-8, uncertified by the orthogonality test),
measured on the CPU by tests/test_refit_reference_host.py, which prints them and holds these records within a factor of two:
    M = MEASURED_M = 0.22 (measured 0.212, B/T129[3]),  M_c = MEASURED_MC = 0.17 (measured 0.164, B/T129[0])
The exact minimisers are slow to compute at 50 digits in pure Python (seconds per problem), so tests/golden/refit_minimisers.json
records them (`python tests/refit_reference.py` writes it); the host test recomputes a sample from the start and checks every
record for stationarity at 50 digits.  Where 50 digits cannot certify orth <= 1e-30 -- F no longer decreases within its own
rounding -- the run ends STALLED or at its 200 steps with orth <= 1e-20 (REF_ORTH), P orth^2 / lmin of which the bound does not feel.
"""
import json
import os
import sys
from functools import lru_cache

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expr_reference as er  # noqa: E402
import score_reference as sr  # noqa: E402
from score_reference import GOLDEN, ROOT, TILE, U  # noqa: E402

sys.path.insert(0, ROOT)

DPS = 50
MAX_PARAMS, MU0, MU_MIN, MU_MAX = 8, 1e-3, 1e-12, 1e12
CONVERGED, MAX_ITER, STALLED, NONFINITE, NO_PARAMS = range(5)
MINIMISERS = os.path.join(GOLDEN, "refit_minimisers.json")
REF_ORTH = 1e-20
# the NumPy restatement against 50 digits, in the units E and E_j of the module text (measured; see there)
MEASURED_M, MEASURED_MC = 0.22, 0.17

OP = {"PUSH_C": 0, "PUSH_F": 1, "ADD": 2, "SUB": 3, "MUL": 4, "DIV": 5, "NEG": 6, "SIN": 7, "COS": 8, "TANH": 9, "ABS": 10,
      "SQUARE": 11, "EXP": 12, "LOG": 13, "SQRT": 14, "POW": 15, "POWI": 16, "SAFE_LOG": 17, "SAFE_SQRT": 18}


def compile_row(text, F=18):
    """(code, constants) of one row by the product's compiler."""
    from rovmpc.expr import compile_expression
    consts = []
    return list(compile_expression(text, consts, F).code), np.array(consts, dtype=np.float64)


class NpMath:
    sin, cos, tanh, exp, log, sqrt, abs, sign = np.sin, np.cos, np.tanh, np.exp, np.log, np.sqrt, np.abs, np.sign
    pow = staticmethod(lambda a, b: np.power(a, b))
    num = staticmethod(float)
    eps5 = 1e-5


class MpMath:
    """Real functions: outside the domain NaN (mpmath would go complex), as in fp64."""
    sin, cos, tanh, exp = mp.sin, mp.cos, mp.tanh, mp.exp
    log = staticmethod(lambda a: mp.log(a) if a > 0 else (mp.ninf if a == 0 else mp.nan))
    sqrt = staticmethod(lambda a: mp.sqrt(a) if a >= 0 else mp.nan)
    abs = staticmethod(abs)
    sign = staticmethod(lambda a: mp.sign(a))
    pow = staticmethod(lambda a, b: mp.power(a, b) if (a > 0 or (a < 0 and b == mp.floor(b))) else (mp.nan if a != 0 or b <= 0 else mp.mpf(0)))
    num = staticmethod(lambda v: mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v)
    eps5 = mp.mpf(1e-5)                                    # the double 1e-5, as the device adds it


def _powi(b, e, one):
    ae, r = abs(e), one
    while ae:
        if ae & 1:
            r = r * b
        b = b * b
        ae >>= 1
    return one / r if e < 0 else r


def dual_eval(code, consts, free_idx, feat, M):
    """(value, [tangent along free constant j]) of the program: interp_eval's operations and the tangent table of the law.
    `feat[k]`: feature k (an array over the rows for NumPy, a number for mpmath); `consts`: numbers of M's kind."""
    P = len(free_idx)
    zero, one = M.num(0.0), M.num(1.0)
    st = []
    for ins in code:
        op, arg = ins & 0xFF, ins >> 8
        if op == OP["PUSH_C"]:
            st.append((consts[arg], [one if arg == k else zero for k in free_idx]))
        elif op == OP["PUSH_F"]:
            st.append((feat[arg], [zero] * P))
        elif op in (OP["ADD"], OP["SUB"], OP["MUL"], OP["DIV"], OP["POW"]):
            b, db = st.pop()
            a, da = st.pop()
            if op == OP["ADD"]:
                st.append((a + b, [x + y for x, y in zip(da, db)]))
            elif op == OP["SUB"]:
                st.append((a - b, [x - y for x, y in zip(da, db)]))
            elif op == OP["MUL"]:
                st.append((a * b, [x * b + a * y for x, y in zip(da, db)]))
            elif op == OP["DIV"]:
                q = a / b
                st.append((q, [(x - q * y) / b for x, y in zip(da, db)]))
            else:
                st.append((M.pow(a, b), [x * b * M.pow(a, b - one) for x in da]))
        else:
            a, da = st.pop()
            if op == OP["NEG"]:
                st.append((-a, [-x for x in da]))
            elif op == OP["SIN"]:
                c = M.cos(a); st.append((M.sin(a), [x * c for x in da]))
            elif op == OP["COS"]:
                s = M.sin(a); st.append((M.cos(a), [-(x * s) for x in da]))
            elif op == OP["TANH"]:
                t = M.tanh(a); st.append((t, [x * (one - t * t) for x in da]))
            elif op == OP["ABS"]:
                s = M.sign(a); st.append((M.abs(a), [x * s for x in da]))
            elif op == OP["SQUARE"]:
                st.append((a * a, [(2 * a) * x for x in da]))
            elif op == OP["EXP"]:
                e = M.exp(a); st.append((e, [x * e for x in da]))
            elif op == OP["LOG"]:
                st.append((M.log(a), [x / a for x in da]))
            elif op == OP["SQRT"]:
                s = M.sqrt(a); st.append((s, [x / (2 * s) for x in da]))
            elif op == OP["POWI"]:
                e = arg - (1 << 24) if arg >= (1 << 23) else arg
                f = zero if e == 0 else e * _powi(a, e - 1, one)
                st.append((_powi(a, e, one), [f * x for x in da]))
            elif op == OP["SAFE_LOG"]:
                s = M.abs(a) + M.eps5; g = M.sign(a); st.append((M.log(s), [x * g / s for x in da]))
            elif op == OP["SAFE_SQRT"]:
                s = M.sqrt(M.abs(a)); g = M.sign(a); st.append((s, [x * g / (2 * s) for x in da]))
            else:
                raise ValueError("opcode %d" % op)
    (v, dv), = st
    return v, dv


# ---- the sums -------------------------------------------------------------------------------------------------------------------
def _lane_sum(chunks):
    """The law's sum of terms given per recording: lane j adds its terms j, j + TILE, ... of recording after recording from +0,
    then the tree.  (law_sum's reshape is that order within one recording; the lanes carry on into the next.)"""
    acc = np.zeros(TILE)
    with np.errstate(all="ignore"):
        for t in chunks:
            t = np.asarray(t, dtype=np.float64)
            rows = np.concatenate([t, np.zeros((-len(t)) % TILE)]).reshape(-1, TILE)
            live = np.concatenate([np.ones(len(t), bool), np.zeros((-len(t)) % TILE, bool)]).reshape(-1, TILE)
            for row, on in zip(rows, live):
                acc = np.where(on, acc + row, acc)
        s = TILE // 2
        while s:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s //= 2
    return float(acc[0])


def sums_np(code, consts, free_idx, recs):
    """(F, A, g, whether J is finite) in fp64 by the law; recs: [(X (n, F), target (n,))] in the group's order."""
    P = len(free_idx)
    with np.errstate(all="ignore"):
        ev = [dual_eval(code, [float(c) for c in consts], free_idx, [X[:, k] for k in range(X.shape[1])], NpMath) for X, _ in recs]
        p = [np.broadcast_to(v, (len(X),)).astype(np.float64) for (v, _), (X, _) in zip(ev, recs)]
        J = [[np.broadcast_to(np.asarray(d, dtype=np.float64), (len(X),)) for d in dv] for (_, dv), (X, _) in zip(ev, recs)]
        F = _lane_sum([(g - pp) * (g - pp) for pp, (_, g) in zip(p, recs)])
        r = [pp - g for pp, (_, g) in zip(p, recs)]
        A = [[_lane_sum([Jb[j] * Jb[k] for Jb in J]) if k <= j else 0.0 for k in range(P)] for j in range(P)]
        gr = [_lane_sum([Jb[j] * rb for Jb, rb in zip(J, r)]) for j in range(P)]
    finite = all(np.isfinite(Jb[j]).all() for Jb in J for j in range(P))
    return F, A, gr, finite


def sums_mp(code, consts, free_idx, recs):
    """The same sums at the working precision of mpmath (exact sums: the order does not matter there)."""
    P = len(free_idx)
    F, A, g = mp.mpf(0), [[mp.mpf(0)] * P for _ in range(P)], [mp.mpf(0)] * P
    p2 = mp.mpf(0)
    try:
        for X, tgt in recs:
            for xi, gi in zip(X, tgt):
                v, dv = dual_eval(code, consts, free_idx, [mp.mpf(float(x)) for x in xi], MpMath)
                r = v - mp.mpf(float(gi))
                F += r * r; p2 += v * v
                for j in range(P):
                    g[j] += dv[j] * r
                    for k in range(j + 1):
                        A[j][k] += dv[j] * dv[k]
    except (ZeroDivisionError, ValueError):
        return mp.nan, A, g, False, p2
    finite = all(mp.isfinite(x) for row in A for x in row) and all(mp.isfinite(x) for x in g)
    return F, A, g, finite, p2


# ---- the solver (one text for both arithmetics: Python floats are IEEE doubles, rounded operation by operation) ------------------
def _orth(A, g, F, P, sqrt):
    if F == 0:
        return 0 * F
    o = 0 * F
    for j in range(P):
        if A[j][j] > 0:
            v = abs(g[j]) / sqrt(A[j][j] * F)
            o = v if (v > o or v != v) else o
    return o


def _solve(A, g, mu, P, sqrt):
    L = [[0] * P for _ in range(P)]
    for j in range(P):
        for k in range(j + 1):
            s = A[j][k]
            if k == j:
                s = s + mu * s
            for m in range(k):
                s = s - L[j][m] * L[k][m]
            if k == j:
                if not s > 0:
                    return None
                L[j][j] = sqrt(s)
            else:
                L[j][k] = s / L[k][k]
    d = [0] * P
    for j in range(P):
        s = -g[j]
        for m in range(j):
            s = s - L[j][m] * d[m]
        d[j] = s / L[j][j]
    for j in reversed(range(P)):
        s = d[j]
        for m in range(j + 1, P):
            s = s - L[m][j] * d[m]
        d[j] = s / L[j][j]
    return d


def _lm(fun, c0, free_idx, n, max_iter, gtol, xtol, num, sqrt, isfinite):
    """The law's iteration.  fun(c) -> (F, A, g, J finite).  Returns a dict; `sums`: (F, A, g) at the returned constants."""
    P = len(free_idx)
    c = [num(v) for v in c0]
    F, A, g, ok = fun(c)
    out = dict(consts=c, loss0=F / n, loss=F / n, orth=num(0.0), iters=0, status=NO_PARAMS, n_params=P, sums=(F, A, g), mu=None)
    if P == 0:
        return out
    if not (isfinite(F) and ok):
        out.update(loss=num(float("nan")), orth=num(float("nan")), status=NONFINITE)
        return out
    mu, it, status = num(MU0), 0, MAX_ITER
    while True:
        orth = _orth(A, g, F, P, sqrt)
        if F == 0 or orth <= gtol:
            status = CONVERGED
            break
        d = None
        while d is None:
            if mu > MU_MAX:
                status = STALLED
                break
            if it == max_iter:
                status = MAX_ITER
                break
            it += 1
            d = _solve(A, g, mu, P, sqrt)
            if d is None:
                mu = mu * 10
        if d is None:
            break
        small = all(abs(d[j]) <= xtol * (abs(c[k]) + xtol) for j, k in enumerate(free_idx))
        t = list(c)
        for j, k in enumerate(free_idx):
            t[k] = c[k] + d[j]
        Ft, At, gt, okt = fun(t)
        if isfinite(Ft) and Ft <= F and okt:
            c, F, A, g = t, Ft, At, gt
            mu = max(mu / 10, num(MU_MIN))
        else:
            mu = mu * 10
        if small:
            status = CONVERGED
            break
    out.update(consts=c, loss=F / n, orth=_orth(A, g, F, P, sqrt), iters=it, status=status, sums=(F, A, g), mu=mu)
    return out


def free_indices(code, consts, free=None):
    """The free constants in pool order; default: all but those that occur only as POW exponents (scoring.default_free)."""
    if free is None:
        from rovmpc.scoring import default_free
        free = default_free(code, len(consts))
    return [k for k in range(len(consts)) if free[k]]


def refit_np(text, recs, c0=None, free=None, max_iter=50, gtol=1e-10, xtol=1e-12):
    code, consts = compile_row(text, recs[0][0].shape[1])
    c0 = consts if c0 is None else np.asarray(c0, dtype=np.float64)
    idx = free_indices(code, consts, free)
    n = sum(len(X) for X, _ in recs)
    return _lm(lambda c: sums_np(code, c, idx, recs), c0, idx, float(n), max_iter, gtol, xtol, float, np.sqrt, np.isfinite)


def refit_mp(text, recs, c0=None, free=None, max_iter=200, gtol=mp.mpf("1e-30"), xtol=0):
    """The exact minimiser from the start at 50 digits; `extra`: |p|^2, lmin of the diag-scaled A and diag A there."""
    code, consts = compile_row(text, recs[0][0].shape[1])
    c0 = consts if c0 is None else np.asarray(c0, dtype=np.float64)
    idx = free_indices(code, consts, free)
    n = sum(len(X) for X, _ in recs)
    with mp.workdps(DPS):
        last = {}

        def fun(c):
            F, A, g, ok, p2 = sums_mp(code, c, idx, recs)
            last[tuple(c)] = p2
            return F, A, g, ok
        out = _lm(fun, c0, idx, mp.mpf(n), max_iter, gtol, mp.mpf(xtol), MpMath.num, mp.sqrt, mp.isfinite)
        F, A, g = out["sums"]
        P = len(idx)
        out["p2"] = last.get(tuple(out["consts"]), mp.mpf(0))
        out["diag"] = [A[j][j] for j in range(P)]
        out["lmin"], out["full_rank"] = scaled_lmin(A, P)
        out["free_idx"] = idx
    return out


RANK_TOL = 1e-10


def scaled_lmin(A, P):
    """(smallest eigenvalue of D^-1 A D^-1 above P RANK_TOL, whether all are above it), D = diag(A)^(1/2), in fp64.  g = J^T r lies
    in the range of A = J^T J, so on a rank-deficient A (a product of two constants) the bound on F holds with the smallest
    eigenvalue of the range; the constants themselves are then not determined.  (0, False) where a diagonal entry is 0."""
    if P == 0:
        return 0.0, False
    a = np.array([[float(A[max(j, k)][min(j, k)]) for k in range(P)] for j in range(P)])
    d = np.sqrt(np.diag(a))
    if not (d > 0).all():
        return 0.0, False
    w = np.linalg.eigvalsh(a / np.outer(d, d))
    live = w[w > P * RANK_TOL]
    return (float(live[0]) if len(live) else 0.0), bool(len(live) == P)


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def _gamma(k):
    return k * U / (1 - k * U)


def loss_bound(rec, gtol=1e-10, M=None):
    """The largest loss a converged fit may report against record `rec` of the exact minimiser (module text)."""
    M = MEASURED_M if M is None else M
    Fs, n, P, p = float(rec["F"]), rec["n"], rec["P"], np.sqrt(float(rec["p2"]))
    derived = Fs * ((P * gtol ** 2 / rec["lmin"] if rec["lmin"] > 0 else np.inf) + _gamma(n + 2) + U)
    E = 2 * U * p * np.sqrt(Fs) + (U * p) ** 2
    return (Fs + derived + 4 * M * E) / n, derived / n, E / n


def const_bounds(rec, gtol=1e-10, Mc=None):
    """Per free constant: the largest |c_j - c*_j| of a converged fit (module text)."""
    Mc = MEASURED_MC if Mc is None else Mc
    Fs, P, p, lmin = float(rec["F"]), rec["P"], np.sqrt(float(rec["p2"])), rec["lmin"]
    out = []
    for ajj in rec["diag"]:
        if not (rec["full_rank"] and lmin > 0 and ajj > 0):
            out.append((np.inf, np.inf, np.inf))
            continue
        derived = np.sqrt(P * Fs) * gtol / (lmin * np.sqrt(ajj))
        Ej = U * p / np.sqrt(lmin * ajj)
        out.append((derived + 4 * Mc * Ej, derived, Ej))
    return out


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
class Problem:
    """One fit: a row, its recordings [(X, target)], the start, the free mask (None: the default)."""

    def __init__(self, name, text, recs, c0, free=None, c_true=None):
        self.name, self.text, self.recs, self.c0, self.free, self.c_true = name, text, recs, np.asarray(c0, dtype=np.float64), free, c_true


def _start(c_true, seed):
    """+-20 % off, the signs from the seed."""
    s = np.random.default_rng(seed).choice([-1.0, 1.0], len(c_true))
    return np.asarray(c_true, dtype=np.float64) * (1.0 + 0.2 * s)


@lru_cache(maxsize=None)
def fixture_a():
    """The 36 generation-1 rows that have constants, each on the recorded table (T = 200: one full tile and a partial one)
    against its own prediction with the file's constants plus 1e-3 std N(0, 1) (default_rng(3000 + k)), from a start +-20 %
    off (signs from default_rng(4000 + k)); k counts the rows of both fronts."""
    d = np.load(os.path.join(GOLDEN, "kat_replay.npz"))
    eqs = json.load(open(os.path.join(GOLDEN, "equations.json")))
    X = np.ascontiguousarray(d["Xs"], dtype=np.float64)
    out, k = [], 0
    for key in ("dtheta_dt", "dgamma_dt"):
        for i, row in enumerate(eqs[key]["rows"]):
            text = row["sympy_format"]
            _, c_true = compile_row(text)
            if len(c_true) == 0:
                continue
            clean = sr.predict_np(text, X)
            target = clean + 1e-3 * np.std(clean) * np.random.default_rng(3000 + k).standard_normal(len(clean))
            out.append(Problem("A/%s[%d]" % (key, i), text, [(X, target)], _start(c_true, 4000 + k), c_true=c_true))
            k += 1
    return out


B_SINE, B_PRODUCT, B_NONE = "0.7*sin(1.3*x3 + 0.4)", "1.5*2.0*x3", "x15 - x17"


def b_deep():
    """The deep expression of expr_reference (16 stack slots) with two of its operands replaced by constants."""
    names = ["x%d" % (i % 9) for i in range(er.MAX_STACK)]
    names[5], names[12] = "0.37", "1.9"
    text = names[-1]
    for nm in reversed(names[:-1]):
        text = "%s - (%s)" % (nm, text)
    return text


B_ROWS = (B_SINE, B_PRODUCT, B_NONE, b_deep())
B_LENGTHS = sr.B_LENGTHS


@lru_cache(maxsize=None)
def fixture_b(T):
    """Per row of B_ROWS a Problem on score_reference.fixture_b(T): noise-free targets (the row itself with its own constants,
    evaluated by NumPy), starts +-20 % off (signs from default_rng(5000 + 10 T + r))."""
    rec = sr.fixture_b(T)
    out = []
    for r, text in enumerate(B_ROWS):
        _, c_true = compile_row(text)
        out.append(Problem("B/T%d[%d]" % (T, r), text, [(rec.X, sr.predict_np(text, rec.X))], _start(c_true, 5000 + 10 * T + r), c_true=c_true))
    return out


def frozen_sine(T=2 * TILE + 3):
    """The sine row with its frequency frozen at the (wrong) start, against score_reference.fixture_b(T)'s noisy target plus
    the row: a two-parameter fit with a residual."""
    rec = sr.fixture_b(T)
    p = fixture_b(T)[0]
    _, c_true = compile_row(B_SINE)
    target = p.recs[0][1] + rec.target * 0.1
    code, consts = compile_row(B_SINE)
    free = [float(c) != 1.3 for c in consts]
    return Problem("B/frozen_sine", B_SINE, [(rec.X, target)], p.c0, free=free, c_true=c_true)


def all_problems():
    out = list(fixture_a())
    for T in B_LENGTHS:
        out += fixture_b(T)
    out.append(frozen_sine())
    return out


# ---- the records of the exact minimisers ----------------------------------------------------------------------------------------
def record_of(problem):
    """The 50-digit run of one problem as JSON-able values (numbers that the bound needs to more than a double: strings)."""
    m = refit_mp(problem.text, problem.recs, problem.c0, problem.free)
    with mp.workdps(DPS):
        return dict(name=problem.name, status=int(m["status"]), iters=int(m["iters"]), P=m["n_params"], n=int(sum(len(X) for X, _ in problem.recs)),
                    consts=[mp.nstr(c, 40) for c in m["consts"]], F=mp.nstr(m["sums"][0], 40), orth=float(m["orth"]), p2=mp.nstr(m["p2"], 20),
                    lmin=m["lmin"], full_rank=m["full_rank"], diag=[float(x) for x in m["diag"]], free_idx=list(m["free_idx"]))


@lru_cache(maxsize=None)
def minimisers():
    """name -> record, from tests/golden/refit_minimisers.json."""
    return {r["name"]: r for r in json.load(open(MINIMISERS))}


def star_consts(rec):
    with mp.workdps(DPS):
        return [mp.mpf(s) for s in rec["consts"]]


if __name__ == "__main__":
    from concurrent.futures import ProcessPoolExecutor
    probs = all_problems()
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        recs = list(ex.map(record_of, probs))
    json.dump(recs, open(MINIMISERS, "w"), indent=0)
    for r in recs:
        print(r["name"], r["status"], r["iters"], r["P"], r["F"][:12], r["orth"], r["lmin"])
