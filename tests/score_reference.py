"""The scores of rovmpc_score_rows (include/rovmpc.h) restated in NumPy and at 50 digits, their error bounds, and the fixtures
of tests/test_score_reference_host.py and tests/test_score_gpu.py.

score_np    the law in NumPy, in the law's own summation order (TILE partial sums over i = j, j + TILE, ..., then the tree).
score_true  the eight columns at 50 digits (mpmath) FROM GIVEN fp64 ARRAYS est, truth, pred, target.  Only the metric arithmetic
            is new ground: the arithmetic of est is rovmpc_replay's, pinned by its own tests and by the bit law.
score_bounds  first-order rounding bounds on the columns, derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u), any
            summation order of n terms:
              SS_res    each term fl(fl(y - e)^2) carries 2 roundings, the sum n - 1:  |dSS_res| <= gamma_{n+2} SS_res
              SS_tot    ybar carries |d ybar| <= delta = gamma_n max|y| (n - 1 additions and the division).  The shift is the same
                        for every i and sum (y_i - ybar) = 0, so it enters only in second order, n delta^2:
                        |dSS_tot| <= gamma_{n+2} (SS_tot + n delta^2) + n delta^2
              r2        q = SS_res / SS_tot: |dq| <= q (dSS_res / SS_res + dSS_tot / SS_tot + u); r2 = fl(1 - q): + u |r2|
              rmse      sqrt halves the relative error of SS_res / n (gamma_{n+2} + u) and adds its own rounding u
              loss      gamma_{n+2} + u, relative; r2_deriv as r2 on (g, p)
              max_abs, last   one rounding: u |v|;   ss_res as SS_res;   n_finite exact
            Every bound is doubled for the dropped second-order terms.  A column passes when error / bound <= 1.
"""
import json
import os
import re
from functools import lru_cache

import mpmath as mp
import numpy as np

import expr_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DPS = 50
U = 2.0 ** -53
COLS = ("r2", "rmse", "max_abs", "n_finite", "loss", "r2_deriv", "last", "ss_res")
RK4, EULER, DOUBLE_EULER, TRAPEZOID = 0, 1, 2, 3
INTEGRATORS = (RK4, EULER, DOUBLE_EULER, TRAPEZOID)


def header_define(name):
    hdr = open(os.path.join(ROOT, "include", "rovmpc.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))


TILE = header_define("ROVMPC_SCORE_TILE")


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---- the replay in NumPy (for the ranking and the place where a row turns non-finite; its bits are not the law's) ------------
def predict_np(text, X):
    from oracle import rovmpc_oracle as orc
    X = np.asarray(X, dtype=np.float64)
    out = orc.SymbolicModel(text.strip().replace("^", "**"), n_features=X.shape[1])([X[:, i] for i in range(X.shape[1])])
    return np.broadcast_to(np.asarray(out, dtype=np.float64), (X.shape[0],)).copy()


def replay_np(text, X, time, y0, integrator):
    """(est, pred) of one row on one recording by the references named in include/rovmpc.h."""
    X, time = np.asarray(X, dtype=np.float64), np.asarray(time, dtype=np.float64)
    T = len(time)
    p = predict_np(text, X)
    est = np.empty(T)
    est[0] = y0
    with np.errstate(all="ignore"):
        if integrator in (RK4, EULER):
            dt = np.diff(time)
            if integrator == RK4 and T > 1:
                k2 = predict_np(text, (X[:-1] + X[1:]) / 2)
                inc = (dt / 6) * (p[:-1] + 2 * k2 + 2 * k2 + p[1:])
            else:
                inc = p[:-1] * dt
            est = np.cumsum(np.concatenate([[y0], inc]))                 # sequential, left to right
        else:
            y, w = float(y0), 0.0
            for i in range(1, T):
                dt = time[i] - time[i - 1]
                if integrator == DOUBLE_EULER:
                    y = y + w * dt
                    w = w + p[i - 1] * dt
                else:
                    w = w + (p[i - 1] + p[i]) / 2 * dt
                    y = y + dt * w
                est[i] = y
    return est, p


# ---- the law in NumPy -----------------------------------------------------------------------------------------------------------
def law_sum(terms, tile=None):
    """TILE partial sums, partial j over the terms j, j + TILE, ... in increasing order from +0, then v[j] += v[j + s]."""
    tile = tile or TILE
    t = np.asarray(terms, dtype=np.float64)
    pad = (-len(t)) % tile
    rows = np.concatenate([t, np.zeros(pad)]).reshape(-1, tile)
    acc = np.zeros(tile)
    with np.errstate(all="ignore"):
        for row in rows:
            acc = acc + row
        s = tile // 2
        while s:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s //= 2
    return float(acc[0])


def _r2(ss_res, ss_tot, n):
    if n < 2:
        return np.nan
    if ss_tot == 0.0:
        return 1.0 if ss_res == 0.0 else (np.nan if np.isnan(ss_res) else 0.0)
    with np.errstate(all="ignore"):
        return float(1.0 - np.float64(ss_res) / np.float64(ss_tot))


def score_np(est, truth, pred=None, target=None, n=None, tile=None, mutant=None):
    """The eight columns from est, truth, pred, target (first n entries).  `mutant`: a deliberately wrong variant for the
    tests of the bound -- "one_pass" takes SS_tot as sum y^2 - (sum y)^2 / n, "about_zero" takes it about 0."""
    n = len(truth) if n is None else int(n)
    e, y = np.asarray(est, dtype=np.float64)[:n], np.asarray(truth, dtype=np.float64)[:n]
    out = np.full(8, np.nan)
    fin = np.isfinite(e)
    nf = n if fin.all() else int(np.argmin(fin))
    out[3] = nf
    with np.errstate(all="ignore"):
        if nf == n:
            d = y - e
            ss_res = law_sum(d * d, tile)
            if mutant == "one_pass":
                sy = law_sum(y, tile)
                ss_tot = law_sum(y * y, tile) - sy * sy / n
            elif mutant == "about_zero":
                ss_tot = law_sum(y * y, tile)
            else:
                c = y - law_sum(y, tile) / n
                ss_tot = law_sum(c * c, tile)
            out[0], out[1], out[2] = _r2(ss_res, ss_tot, n), np.sqrt(np.float64(ss_res) / n), np.max(np.abs(d)) if not np.isnan(d).any() else np.nan
            out[6], out[7] = e[n - 1], ss_res
        if target is not None and pred is not None:
            p, g = np.asarray(pred, dtype=np.float64)[:n], np.asarray(target, dtype=np.float64)[:n]
            if np.isfinite(p).all():
                dp, cg = g - p, g - law_sum(g, tile) / n
                ss_resp = law_sum(dp * dp, tile)
                out[4], out[5] = ss_resp / n, _r2(ss_resp, law_sum(cg * cg, tile), n)
    return out


# ---- 50 digits ------------------------------------------------------------------------------------------------------------------
def _gamma(k):
    return k * U / (1 - k * U)


def _pair_true(y, e, n):
    """(SS_res, SS_tot, max |y - e|, max |y|) exact from fp64 arrays."""
    ym = [mp.mpf(float(v)) for v in y[:n]]
    em = [mp.mpf(float(v)) for v in e[:n]]
    ybar = mp.fsum(ym) / n
    return (mp.fsum((a - b) ** 2 for a, b in zip(ym, em)), mp.fsum((a - ybar) ** 2 for a in ym),
            max(abs(a - b) for a, b in zip(ym, em)), max(abs(a) for a in ym))


def _r2_true_bound(ss_res, ss_tot, ymax, n):
    """(exact r2 or None where the law's value hangs on a rounded zero, bound)."""
    if n < 2:
        return mp.nan, 0.0
    if ss_tot == 0:
        return None, np.inf
    q = ss_res / ss_tot
    delta = _gamma(n) * ymax
    b_tot = _gamma(n + 2) * (ss_tot + n * delta ** 2) + n * delta ** 2
    r2 = 1 - q
    return r2, float(q * (_gamma(n + 2) + b_tot / ss_tot + U) + U * abs(r2))


def score_true(est, truth, pred=None, target=None, n=None):
    """(values, bounds): the eight columns at 50 digits from the given fp64 arrays and the doubled first-order bounds.  A NaN
    value means the law asks for NaN; a value of None (bound inf) means the law's value is not determined by exact arithmetic
    (SS_tot exactly 0: the caller compares with score_np instead)."""
    n = len(truth) if n is None else int(n)
    e, y = np.asarray(est, dtype=np.float64)[:n], np.asarray(truth, dtype=np.float64)[:n]
    val, bnd = [mp.nan] * 8, [0.0] * 8
    fin = np.isfinite(e)
    nf = n if fin.all() else int(np.argmin(fin))
    val[3] = mp.mpf(nf)
    with mp.workdps(DPS):
        if nf == n and np.isfinite(y).all():
            ss_res, ss_tot, mx, ymax = _pair_true(y, e, n)
            val[0], bnd[0] = _r2_true_bound(ss_res, ss_tot, ymax, n)
            val[1] = mp.sqrt(ss_res / n); bnd[1] = float(val[1] * ((_gamma(n + 2) + U) / 2 + U))
            val[2] = mx; bnd[2] = float(U * mx)
            val[6] = mp.mpf(float(e[n - 1])); bnd[6] = float(U * abs(val[6]))
            val[7] = ss_res; bnd[7] = float(_gamma(n + 2) * ss_res)
        if target is not None and pred is not None:
            p, g = np.asarray(pred, dtype=np.float64)[:n], np.asarray(target, dtype=np.float64)[:n]
            if np.isfinite(p).all() and np.isfinite(g).all():
                ss_resp, ss_totg, _, gmax = _pair_true(g, p, n)
                val[4] = ss_resp / n; bnd[4] = float(val[4] * (_gamma(n + 2) + U))
                val[5], bnd[5] = _r2_true_bound(ss_resp, ss_totg, gmax, n)
    return val, [2.0 * b for b in bnd]


def score_ratios(got, est, truth, pred=None, target=None, n=None):
    """error / bound per column for the eight values `got`: 0 where a NaN or an exact value is matched, inf where it is
    missed, NaN where exact arithmetic does not determine the law's value (score_true)."""
    val, bnd = score_true(est, truth, pred, target, n)
    out = np.zeros(8)
    with mp.workdps(DPS):
        for k in range(8):
            g = float(got[k])
            if val[k] is None:
                out[k] = np.nan
            elif mp.isnan(val[k]):
                out[k] = 0.0 if np.isnan(g) else np.inf
            elif not np.isfinite(g):
                out[k] = np.inf
            else:
                err = abs(mp.mpf(g) - val[k])
                out[k] = 0.0 if err == 0 else (float(err / bnd[k]) if bnd[k] > 0 else np.inf)
    return out


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
class Recording:
    def __init__(self, X, time, truth, target, y0):
        self.X, self.time, self.truth, self.target, self.y0 = X, time, truth, target, float(y0)


@lru_cache(maxsize=None)
def fixture_a():
    """The recorded replay table (T = 200, non-uniform time) with all 23 + 14 generation-1 rows: {"theta" / "gamma":
    (row texts, Recording, index of the reference's chosen row)}.  truth = the file's RK4 replay of the chosen rows plus
    1e-3 std N(0, 1) (default_rng(1) for each series); target = the chosen row's own prediction."""
    d = np.load(os.path.join(GOLDEN, "kat_replay.npz"))
    eqs = json.load(open(os.path.join(GOLDEN, "equations.json")))
    out = {}
    for name, key, series, y0 in (("theta", "dtheta_dt", "rk4_theta", "theta0"), ("gamma", "dgamma_dt", "rk4_gamma", "gamma0")):
        rows = eqs[key]["rows"]
        texts = [r["sympy_format"] for r in rows]
        chosen = [r["complexity"] for r in rows].index(eqs[key]["chosen_complexity"])
        clean = np.asarray(d[series], dtype=np.float64)
        truth = clean + 1e-3 * np.std(clean) * np.random.default_rng(1).standard_normal(len(clean))
        target = predict_np(texts[chosen], d["Xs"])
        out[name] = (texts, Recording(np.ascontiguousarray(d["Xs"]), np.ascontiguousarray(d["time"]), truth, target, float(d[y0])), chosen)
    return out


B_ROWS = ("x15 - x17", er.deep_expression(), "log(x3)")
B_LENGTHS = (1, 2, TILE, TILE + 1, 2 * TILE + 3)


@lru_cache(maxsize=None)
def fixture_b(T):
    """Synthetic scaled rows N(0, 1), time = cumsum U(0.005, 0.03); truth a slow random walk, target N(0, 0.1)."""
    rng = np.random.default_rng(7000 + T)
    X = rng.standard_normal((T, 18))
    time = np.cumsum(rng.uniform(0.005, 0.03, T))
    truth = 0.3 + np.cumsum(0.01 * rng.standard_normal(T))
    target = 0.1 * rng.standard_normal(T)
    return Recording(X, time, truth, target, truth[0])
