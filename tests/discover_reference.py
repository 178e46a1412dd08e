"""rovmpc_discover_rows (include/rovmpc.h) restated in NumPy, its exact counterparts, the bounds, and the fixtures of
tests/test_discover_reference_host.py, tests/test_discover_host.py and tests/test_discover_gpu.py.

select_np     stage 2 of the law operation by operation on a given packed Gram: np.float64 scalars, one rounding each, the
              law's order.  Given the device's Gram its outputs are the device's, bit for bit.
gram_exact    the exact Gram of given double columns as an unevaluated pair hi + lo: every product split by the error-free
              two-product (Veltkamp / Dekker), every sum by math.fsum, which is exact.  No 50-digit arithmetic.
exact_state   what stage 2 computes, from the exact Gram at 50 digits (mpmath): for a picked set the Schur complement
              rho_j, q_j of every other term, the coefficients a = G_PP^-1 b_P and F = c - b_P.a.
greedy_lstsq  an independent forward selection on the columns themselves: every candidate re-solved by np.linalg.lstsq.

Bounds.  u = 2^-53, gamma_k = k u / (1 - k u).
  Gram.  An entry is a sum of n products in some order, each product and each partial sum rounded at most once (a fused
    multiply-add rounds once for both); a chunk of m rows and the nc - 1 additions of the other chunks give a term at most
    m + nc - 1 <= n roundings.  So for any order, fused or not:   |G^_jk - G_jk| <= gamma_{n+1} sum_i |v_j(i) v_k(i)|,
    and by Cauchy-Schwarz <= gamma_{n+1} sqrt(G_jj G_kk): every entry of the diagonally scaled Gram moves by at most eps.
  Stage 2, to first order in an entrywise scaled perturbation eps.  With P the picked set, beta_j = G_PP^-1 G_Pj and
    nu_j = sqrt(G_jj) + sum_i |beta_ji| sqrt(G_ii)  (nu for the target: sqrt(c) (1 + |a~|_1), a~_i = a_i sqrt(G_ii / c)):
      rho_j = u_j.G u_j, q_j = u_j.G u_M with u_j = (-beta_j, e_j):   |d rho_j| <= eps nu_j^2,   |d q_j| <= eps nu_j nu_M
      gain_j = q_j^2 / rho_j:      |d gain_j| <= (2 |q_j| |d q_j| + |d q_j|^2) / rho_j + q_j^2 |d rho_j| / rho_j^2
                                   (the square is kept: where the target is all but spanned, q_j is itself a rounding)
      F = c - b_P.a = u_M.G u_M:   |d F| <= eps c (1 + |a~|_1)^2
      a = G_PP^-1 b_P:  d a = G_PP^-1 (d b - dG a), so with lmin the smallest eigenvalue of the scaled picked block
                        |d a_i| <= sqrt(c / G_ii) eps sqrt(k) (1 + |a~|_1) / lmin      (k = |P|)
    Every bound is doubled for the dropped second-order terms.
  eps = gamma_{n+1} + 4 K u.  The first part is the Gram's error, derived.  K u stands for the rounding of stage 2's own
    arithmetic (at most 8 steps of a Cholesky factorisation and a back substitution), which is not derived here: K is the
    largest error of select_np -- on the correctly rounded exact Gram, so that the Gram contributes u / 2 at most --
    against exact_state, over the gains, coefficients and F of every step of fixtures A and B, in units of the forms above
    with eps = u.  Measured on the CPU by tests/test_discover_reference_host.py (never on the GPU), which prints it and holds
    this record within a factor of two:
        K = MEASURED_K = 0.85   (measured 0.829: the gain of term 1 at step 0 of B/ragged_offsets, group 0)
    Steps at which the target is already spanned (exact F <= u c) are left out of K: what is computed there is a rounding.
  A pick is DECIDED where the exact gain of the picked term exceeds that of every other candidate by more than the sum of the
  two bounds on the gains.  The loss of a discovered row as rovmpc_score_rows evaluates it (column 4) differs from the front's
  by dF, by the rounding of the row's own k products and k - 1 sums, |e_i| <= gamma_{k+1} sum_m |a_m v_m(i)|, so |e|_2 <=
  gamma_{k+1} sqrt(c) |a~|_1 and the sum of squares moves by at most 2 sqrt(F) |e| + |e|^2, and by that entry's own summation,
  gamma_{n+2} F (score_reference): loss_bound.
"""
import json
import math
import os
import sys
from functools import lru_cache

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as sr  # noqa: E402
from score_reference import GOLDEN, ROOT, U, same  # noqa: E402,F401

sys.path.insert(0, ROOT)

DPS = 50
MAX_TERMS, MAX_SIZE, CHUNK = (sr.header_define("ROVMPC_DISCOVER_" + n) for n in ("MAX_TERMS", "MAX_SIZE", "CHUNK"))
FULL, MIN_GAIN, EXHAUSTED, NONFINITE = range(4)
MEASURED_K = 0.85
DEFAULTS = dict(max_terms=8, dep_tol=1e-10, min_gain=1e-12)


def _gamma(k):
    return k * U / (1 - k * U)


def tri(j, k):
    return j * (j + 1) // 2 + k if j >= k else k * (k + 1) // 2 + j


def unpack(gram, M):
    """The packed lower triangle as the full symmetric (M + 1, M + 1) matrix."""
    gram = np.asarray(gram, dtype=np.float64)
    return np.array([[gram[tri(j, k)] for k in range(M + 1)] for j in range(M + 1)])


def pack(full):
    C = len(full)
    return np.array([full[j][k] for j in range(C) for k in range(j + 1)], dtype=np.float64)


# ---- stage 2 in NumPy -------------------------------------------------------------------------------------------------------
def select_np(gram, M, n, max_terms=8, dep_tol=1e-10, min_gain=1e-12, mutant=None):
    """Stage 2 of the law on the packed Gram.  Returns dict(picks (S,) int32, coef (S, S), loss (S + 1,), n_sel, status, n) and,
    for the tests, `steps`: per step taken or refused the candidates' gains (NaN where not a candidate).  `mutant`: a
    deliberately wrong law -- "no_division" (gain = q^2), "no_dep_test", "ties_high"."""
    f = np.float64
    S = int(max_terms)
    g = np.asarray(gram, dtype=np.float64)
    G = lambda j, k: f(g[tri(j, k)])
    picks, coef, loss = np.full(S, -1, np.int32), np.zeros((S, S)), np.full(S + 1, np.nan)
    out = dict(picks=picks, coef=coef, loss=loss, n_sel=0, status=FULL, n=int(n), steps=[])
    with np.errstate(all="ignore"):
        c, dn = G(M, M), f(n)
        loss[0] = c / dn
        if not np.isfinite(c):
            out["status"] = NONFINITE
            return out
        adm = [bool(G(j, j) > 0 and np.isfinite(G(j, j)) and np.isfinite(G(M, j))) for j in range(M)]
        rho, q = [G(j, j) for j in range(M)], [G(M, j) for j in range(M)]
        w = [[f(0.0)] * S for _ in range(M)]
        picked, z, order, F = [False] * M, [], [], c
        for s in range(S):
            gains = np.full(M, np.nan)
            for j in range(M):
                if adm[j] and not picked[j] and (mutant == "no_dep_test" or rho[j] > f(dep_tol) * G(j, j)):
                    gains[j] = (q[j] * q[j]) if mutant == "no_division" else (q[j] * q[j]) / rho[j]
            out["steps"].append(gains)
            p = -1
            for j in range(M):
                if gains[j] == gains[j] and (p < 0 or gains[j] > gains[p] or (mutant == "ties_high" and gains[j] == gains[p])):
                    p = j
            if p < 0:
                out["status"] = EXHAUSTED
                break
            if gains[p] <= f(min_gain) * c:
                out["status"] = MIN_GAIN
                break
            l = np.sqrt(rho[p])
            zs = q[p] / l
            for j in range(M):
                if not adm[j] or picked[j]:
                    continue
                if j == p:
                    w[j][s] = l
                    continue
                acc = f(0.0)
                for t in range(s):
                    acc = acc + w[p][t] * w[j][t]
                w[j][s] = (G(p, j) - acc) / l
                rho[j] = rho[j] - w[j][s] * w[j][s]
                q[j] = q[j] - w[j][s] * zs
            picked[p] = True
            order.append(p); z.append(zs)
            F = F - zs * zs
            picks[s] = p
            loss[s + 1] = (F if F > 0 else f(0.0)) / dn
            a = [f(0.0)] * (s + 1)
            for i in range(s, -1, -1):
                acc = f(0.0)
                for m in range(i + 1, s + 1):
                    acc = acc + w[order[m]][i] * a[m]
                a[i] = (z[i] - acc) / w[order[i]][i]
            coef[s, :s + 1] = a
            out["n_sel"] = s + 1
    return out


# ---- the exact Gram ---------------------------------------------------------------------------------------------------------
def _two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker; no overflow or underflow in the fixtures' range)."""
    p = a * b
    split = 134217729.0                                        # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def gram_exact(V):
    """V (n, C): the columns, the last the target.  Returns (hi, lo, absum), each the packed lower triangle: hi + lo is the exact
    Gram to a relative 2^-105 (hi the correctly rounded sum, lo the correctly rounded rest), absum = sum |v_j v_k|."""
    V = np.asarray(V, dtype=np.float64)
    C = V.shape[1]
    E = C * (C + 1) // 2
    hi, lo, ab = np.empty(E), np.empty(E), np.empty(E)
    for j in range(C):
        for k in range(j + 1):
            p, e = _two_product(V[:, j], V[:, k])
            parts = np.concatenate([p, e]).tolist()
            h = math.fsum(parts)
            hi[tri(j, k)], lo[tri(j, k)] = h, math.fsum(parts + [-h])
            ab[tri(j, k)] = math.fsum(np.abs(p).tolist())
    return hi, lo, ab


def gram_ratio(got, V):
    """The largest |got - exact| / (gamma_{n+1} sum |v_j v_k|) over the entries (0 where both are 0), and its entry."""
    hi, lo, ab = gram_exact(V)
    n = len(V)
    worst, at = 0.0, -1
    for e in range(len(hi)):
        err = abs((float(got[e]) - hi[e]) - lo[e])                 # (the first difference is exact: Sterbenz)
        if err == 0:
            continue
        r = err / (_gamma(n + 1) * ab[e]) if ab[e] > 0 else np.inf
        if not r <= worst:
            worst, at = r, e
    return worst, at


# ---- stage 2 exactly --------------------------------------------------------------------------------------------------------
def exact_state(hi, lo, M, picked):
    """At 50 digits from the exact Gram hi + lo, for the picked list P: dict(rho, q (per term, None for the picked), nu (per
    term and, at index M, the target), a, F, lmin (the scaled picked block's smallest eigenvalue, fp64), c, diag)."""
    with mp.workdps(DPS):
        G = lambda j, k: mp.mpf(float(hi[tri(j, k)])) + mp.mpf(float(lo[tri(j, k)]))
        k = len(picked)
        diag = [G(j, j) for j in range(M + 1)]
        c = diag[M]
        if k:
            inv = mp.matrix([[G(a, b) for b in picked] for a in picked]) ** -1
        beta = lambda j: [mp.fsum(inv[i, m] * G(picked[m], j) for m in range(k)) for i in range(k)] if k else []
        rho, q, nu = [None] * M, [None] * M, [None] * (M + 1)
        bM = beta(M)
        for j in range(M + 1):
            if j in picked:
                continue
            bj = bM if j == M else beta(j)
            nu[j] = mp.sqrt(diag[j]) + mp.fsum(abs(bj[i]) * mp.sqrt(diag[picked[i]]) for i in range(k))
            if j < M and diag[j] > 0:
                rho[j] = diag[j] - mp.fsum(bj[i] * G(picked[i], j) for i in range(k))
                q[j] = G(M, j) - mp.fsum(bj[i] * G(picked[i], M) for i in range(k))
        F = c - mp.fsum(bM[i] * G(picked[i], M) for i in range(k))
        lmin = 1.0
        if k:
            blk = np.array([[float(G(a, b) / mp.sqrt(diag[a] * diag[b])) for b in picked] for a in picked])
            lmin = float(np.linalg.eigvalsh(blk)[0])
        return dict(rho=rho, q=q, nu=nu, a=bM, F=F, lmin=lmin, c=c, diag=diag)


def gain_bounds(st, eps):
    """(exact gains, bounds) per term from exact_state (NaN for picked or zero terms); doubled first-order bounds."""
    M = len(st["rho"])
    gains, bnd = np.full(M, np.nan), np.full(M, np.nan)
    with mp.workdps(DPS):
        for j in range(M):
            rho, q = st["rho"][j], st["q"][j]
            if rho is None or not rho > 0:
                continue
            drho, dq = eps * st["nu"][j] ** 2, eps * st["nu"][j] * st["nu"][M]
            gains[j] = float(q * q / rho)
            bnd[j] = 2.0 * float((2 * abs(q) * dq + dq * dq) / rho + q * q * drho / rho ** 2)
    return gains, bnd


def a_tilde_1(st, picked):
    with mp.workdps(DPS):
        return float(mp.fsum(abs(a) * mp.sqrt(st["diag"][p] / st["c"]) for a, p in zip(st["a"], picked))) if st["c"] > 0 else 0.0


def coef_bounds(st, picked, eps):
    """Per picked term the doubled bound on |a_i - exact a_i|."""
    k, a1 = len(picked), a_tilde_1(st, picked)
    return [2.0 * math.sqrt(float(st["c"] / st["diag"][p])) * eps * math.sqrt(k) * (1 + a1) / st["lmin"] for p in picked]


def f_bound(st, picked, eps):
    """The doubled bound on |F - exact F| (the sum of squares, not yet over n)."""
    return 2.0 * eps * float(st["c"]) * (1 + a_tilde_1(st, picked)) ** 2


def eps_total(n):
    return _gamma(n + 1) + 4 * MEASURED_K * U


def loss_bound(st, picked, n):
    """The doubled bound on |front loss - rovmpc_score_rows column 4 of the same row| (module text)."""
    k, c, F = len(picked), float(st["c"]), max(float(st["F"]), 0.0)
    e = _gamma(k + 1) * math.sqrt(c) * a_tilde_1(st, picked)
    return (f_bound(st, picked, eps_total(n)) + 2.0 * (2 * math.sqrt(F) * e + e * e + _gamma(n + 2) * F)) / n


def decided_steps(hi, lo, M, picks, n, eps=None):
    """Per step of `picks` (the reference's own): (decided?, relative gap to the runner-up, relative bound), from exact_state.
    The candidates are all unpicked terms with an exact rho > 0."""
    eps = eps_total(n) if eps is None else eps
    out = []
    for s, p in enumerate(picks):
        gains, bnd = gain_bounds(exact_state(hi, lo, M, list(picks[:s])), eps)
        others = [j for j in range(M) if j != p and gains[j] == gains[j]]
        if not others:
            out.append((True, np.inf, 0.0))
            continue
        margin = min(gains[p] - gains[j] - (bnd[p] + bnd[j]) for j in others)
        second = max(gains[j] for j in others)
        out.append((bool(margin > 0), float((gains[p] - second) / gains[p]), float(max(bnd[p] + bnd[j] for j in others) / gains[p])))
    return out


def measure_k(case_values):
    """The constant K of the module text on one case: select_np on the correctly rounded exact Gram against exact_state, the
    largest error over gains, coefficients and F in units of the bounds' forms with eps = u (undoubled).  `case_values`: (V, M, S)."""
    V, M, S = case_values
    hi, lo, _ = gram_exact(V)
    n = len(V)
    res = select_np(hi, M, n, max_terms=S)
    worst, where = 0.0, ""
    with mp.workdps(DPS):
        for s in range(res["n_sel"] + (1 if res["n_sel"] < S and res["status"] != NONFINITE else 0)):
            picked = [int(p) for p in res["picks"][:s]]
            st = exact_state(hi, lo, M, picked)
            gains, bnd = gain_bounds(st, U)
            for j in range(M if st["F"] > U * st["c"] else 0):          # (a spanned target: the gains are roundings, second order)
                got = res["steps"][s][j]
                if got == got and gains[j] == gains[j] and bnd[j] > 0:
                    r = float(abs(mp.mpf(float(got)) - st["q"][j] ** 2 / st["rho"][j])) / (bnd[j] / 2)
                    if r > worst:
                        worst, where = r, "gain step %d term %d" % (s, j)
        for s in range(res["n_sel"]):
            picked = [int(p) for p in res["picks"][:s + 1]]
            st = exact_state(hi, lo, M, picked)
            for i, b in enumerate(coef_bounds(st, picked, U)):
                r = float(abs(mp.mpf(float(res["coef"][s, i])) - st["a"][i])) / (b / 2)
                if r > worst:
                    worst, where = r, "coef size %d term %d" % (s + 1, i)
            Fnp = res["loss"][s + 1] * n
            if st["F"] > U * st["c"]:                                   # (below that the law clamps a rounding to 0)
                r = float(abs(mp.mpf(float(Fnp)) - st["F"])) / (f_bound(st, picked, U) / 2 + U * Fnp)
                if r > worst:
                    worst, where = r, "F size %d" % (s + 1)
    return worst, where


# ---- an independent selection on the columns ----------------------------------------------------------------------------------
def greedy_lstsq(V, S):
    """Forward selection on the columns V[:, :-1] against V[:, -1]: at every step every unpicked column with a non-zero
    norm is tried, the picked set re-solved by np.linalg.lstsq, the smallest residual wins.  Returns the picks."""
    V = np.asarray(V, dtype=np.float64)
    Phi, g = V[:, :-1], V[:, -1]
    M = Phi.shape[1]
    picks = []
    for _ in range(min(S, M)):
        best, arg = np.inf, -1
        for j in range(M):
            if j in picks or not np.isfinite(Phi[:, j]).all() or not np.any(Phi[:, j]):
                continue
            A = Phi[:, picks + [j]]
            r = g - A @ np.linalg.lstsq(A, g, rcond=None)[0]
            ss = float(r @ r)
            if ss < best:
                best, arg = ss, j
        if arg < 0:
            break
        picks.append(arg)
    return picks


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
class Case:
    """One call: the term texts, X (B, T, F), target (B, T), lengths (B,) or None, groups, max_terms."""

    def __init__(self, name, terms, X, target, lengths=None, groups="pooled", max_terms=8):
        X, target = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(target, dtype=np.float64)
        if X.ndim == 2:
            X, target = X[None], target[None]
        self.name, self.terms, self.X, self.target, self.lengths, self.groups, self.max_terms = name, list(terms), X, target, lengths, groups, max_terms

    def group_ranges(self):
        B = len(self.X)
        if isinstance(self.groups, str):
            return [(0, B)] if self.groups == "pooled" else [(b, b + 1) for b in range(B)]
        return [(int(a), int(b)) for a, b in zip(self.groups[:-1], self.groups[1:])]

    def columns(self, g=0, term_values=None):
        """V (n, M + 1) of group g: the counted rows of its recordings in order, the terms by NumPy (or `term_values`
        (M, B, T), the device's own) and the target."""
        b0, b1 = self.group_ranges()[g]
        rows = []
        for b in range(b0, b1):
            n = self.X.shape[1] if self.lengths is None else int(self.lengths[b])
            with np.errstate(all="ignore"):
                cols = [sr.predict_np(t, self.X[b, :n]) for t in self.terms] if term_values is None else [term_values[m, b, :n] for m in range(len(self.terms))]
            rows.append(np.stack(cols + [self.target[b, :n]], axis=1))
        return np.concatenate(rows, axis=0)


def library(F=18, products=()):
    from rovmpc.scoring import term_library
    return term_library(F, products=products)


A_NOISES = (0.0, 1e-3)
A_SIZES = {"theta": 4, "gamma": 2}


@lru_cache(maxsize=None)
def fixture_a():
    """The recorded table (T = 200, F = 18) with the 55-term library {1, x_i, sin x_i, cos x_i}; the target is the reference's
    chosen theta row, and its chosen gamma row, plus noise of 0 and 1e-3 of the target's std (default_rng(7)).  {(name,
    noise): Case}; `A_EXPECT`: the terms the front must recover and their coefficients."""
    d = np.load(os.path.join(GOLDEN, "kat_replay.npz"))
    eqs = json.load(open(os.path.join(GOLDEN, "equations.json")))
    X = np.ascontiguousarray(d["Xs"], dtype=np.float64)
    out = {}
    for name, key in (("theta", "dtheta_dt"), ("gamma", "dgamma_dt")):
        rows = eqs[key]["rows"]
        text = rows[[r["complexity"] for r in rows].index(eqs[key]["chosen_complexity"])]["sympy_format"]
        clean = sr.predict_np(text, X)
        for noise in A_NOISES:
            target = clean + noise * np.std(clean) * np.random.default_rng(7).standard_normal(len(clean)) if noise else clean
            out[(name, noise)] = Case("A/%s/noise%g" % (name, noise), library(18), X, target)
    return out


C_THETA = 0.048152514
A_EXPECT = {"theta": {"sin(x17)": C_THETA, "sin(x3)": -C_THETA, "x16": -C_THETA, "x3": -C_THETA}, "gamma": {"x15": 1.0, "x17": -1.0}}
B_PRODUCTS = ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (12, 13), (14, 15), (1, 4))


@lru_cache(maxsize=None)
def fixture_b():
    """Shapes.  "M64": 64 terms (the 55 and nine products) on T = 131, one recording (three tiles of 64 rows, the last of 3);
    "ragged_*": 5 terms on B = 3 recordings of T = 2 * 1024 + 3 with lengths 1, 1024 and 2051 (a chunk of one row, a full chunk,
    two full chunks and one of 3 rows; NaN beyond the lengths), pooled, each and with offsets 0, 2, 3; "one": M = F = T = 1."""
    rec = sr.fixture_b(131)
    X = rec.X
    t64 = 0.7 * X[:, 2] - 0.3 * np.sin(X[:, 5]) + 0.2 * X[:, 1] * X[:, 4] + 0.1 + rec.target
    out = {"M64": Case("B/M64", library(18, B_PRODUCTS), X, t64)}
    T = 2 * CHUNK + 3
    rng = np.random.default_rng(7100)
    Xr = rng.standard_normal((3, T, 18))
    terms = ["1.0", "x0", "sin(x1)", "x2*x3", "cos(x4)"]
    tr = 0.5 + 0.8 * Xr[..., 0] - 0.4 * np.sin(Xr[..., 1]) + 0.05 * rng.standard_normal((3, T))
    lengths = np.array([1, CHUNK, T], dtype=np.int64)
    for b, n in enumerate(lengths):
        Xr[b, n:], tr[b, n:] = np.nan, np.nan
    for gname, groups in (("pooled", "pooled"), ("each", "each"), ("offsets", np.array([0, 2, 3], dtype=np.int32))):
        out["ragged_" + gname] = Case("B/ragged_" + gname, terms, Xr, tr, lengths, groups)
    out["one"] = Case("B/one", ["x0"], np.array([[[2.0]]]), np.array([[3.0]]))
    return out


@lru_cache(maxsize=None)
def fixture_c():
    """Degenerate libraries on score_reference.fixture_b(131)."""
    rec = sr.fixture_b(131)
    X = rec.X
    t = 0.5 * X[:, 0] + 0.25 * X[:, 1] - 0.3 * np.sin(X[:, 2]) + 0.2 * rec.target
    nan_t = t.copy(); nan_t[5] = np.nan
    return {
        "duplicate": Case("C/duplicate", ["x0", "x1", "x0", "sin(x2)"], X, t),
        "near_twin": Case("C/near_twin", ["x0", "x1", "x0 + 1e-9*x5", "sin(x2)"], X, t),
        "zero_term": Case("C/zero_term", ["x0", "0.0*x1", "sin(x2)"], X, t),
        "with_log": Case("C/with_log", ["x0", "log(x3)", "x1", "sin(x2)"], X, t),
        "without_log": Case("C/without_log", ["x0", "x1", "sin(x2)"], X, t),
        "nan_target": Case("C/nan_target", ["x0", "x1"], X, nan_t),
        "zero_target": Case("C/zero_target", ["x0", "x1"], X, np.zeros_like(t)),
        "few_terms": Case("C/few_terms", ["x0", "x1"], X, t),
    }


def reference_front(case, g=0, **kw):
    """(select_np on the correctly rounded exact Gram of the NumPy columns, (hi, lo, absum), V) for one group."""
    V = case.columns(g)
    M = len(case.terms)
    grams = gram_exact(V)
    return select_np(grams[0], M, len(V), max_terms=case.max_terms, **kw), grams, V
