"""The closed-loop N-step-ahead skill of rovmpc_score_pairs (include/rovmpc.h) restated in NumPy and at 50 digits, the error
figure the values are held to, and the fixtures of tests/test_horizon_reference_host.py and tests/test_horizon_gpu.py.

horizon_np    the law in NumPy, operation by operation, vectorised over the windows of one (pair, recording): the stage row,
              the four RK4 stages (or Euler's one), the update, the counting rule, the columns with law_sum.
law_sum       the law's summation order: tiles of TILE consecutive windows, inside a tile the tree v[l] += v[l + s] for
              s = TILE / 2, ..., 1, the tile sums added in increasing tile order from +0.
skill_from_pred   the nine columns from GIVEN fp64 predictions: what a side under test must reproduce from its own pred bits
              (columns 4-8 bit for bit; 0-3 to a few roundings, see column_bounds).
horizon_true  the same law at 50 digits (mpmath) for chosen windows, with the scale of every entry.  The inputs -- rows, time,
              truths, scaler, constants -- are exact fp64 values; slopes by expr_reference.Evaluator on the row texts.

The error figure.  An entry pred[w][j] is the start value plus j increments, so its natural scale is
S = |y_s| + sum_{m <= j} |y*_m - y*_{m-1}|, and error = |got - exact| / (u S) with u = 2^-53.  The chain carries an early
rounding forward through the Jacobian of the later steps; no forward bound is derived here.  As the issue sets it, the bound is
measured on the reference: NP_FIGURE is the largest error of horizon_np over the checked windows of all fixtures (recorded,
rounded up to two places, in tests/golden/horizon_bounds.json and measured again by tests/test_horizon_reference_host.py), and
the GPU gets GPU_MARGIN = 4 times that figure: the device's sin / cos / exp carry the few-ulp bounds of DESIGN section 3 where
NumPy's are <= 1 ulp, and the chain carries them forward.  Where exact arithmetic leaves an operation's domain (log of a
negative slot) or the finite range, the entry is compared by what horizon_np gives: finite or not.
"""
import json
import os
from functools import lru_cache

import mpmath as mp
import numpy as np
from mpmath import mpf

import expr_reference as er
import score_reference as sr
from rollout_reference import SlotEvaluator

ROOT = sr.ROOT
GOLDEN = sr.GOLDEN
DPS = 50
U = 2.0 ** -53
RK4, EULER = 0, 1
PREV_INTERP, PREV_HOLD = 0, 1
TILE = sr.header_define("ROVMPC_HORIZON_TILE")
COLS = ("rmse_theta", "rmse_gamma", "max_abs_theta", "max_abs_gamma", "n_ok", "ss_theta", "ss_gamma", "ss_hold_theta", "ss_hold_gamma")
GEN1 = (14, 15, 16, 17, -1, -1)          # theta, gamma, theta_prev, gamma_prev, cos_theta, sin_gamma
GEN2 = (12, 13, -1, -1, 14, 15)
GPU_MARGIN = 4.0
same = sr.same


def bounds():
    return json.load(open(os.path.join(GOLDEN, "horizon_bounds.json")))


def n_windows(n, H, stride):
    return (n - 1 - H) // stride + 1 if n - 1 - H >= 0 else 0


# ---- the law in NumPy -----------------------------------------------------------------------------------------------------------
def law_sum(terms, tile=None):
    """Tiles of TILE consecutive terms (the last padded with +0), the tree inside a tile, the tile sums from +0 in order."""
    tile = tile or TILE
    t = np.asarray(terms, dtype=np.float64)
    pad = (-len(t)) % tile
    rows = np.concatenate([t, np.zeros(pad)]).reshape(-1, tile)
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for row in rows:
            v = row.copy()
            s = tile // 2
            while s:
                v[:s] = v[:s] + v[s:2 * s]
                s //= 2
            total = total + v[0]
    return float(total)


def _model(text, F):
    from oracle import rovmpc_oracle as orc
    return orc.SymbolicModel(text.strip().replace("^", "**"), n_features=F)


def _predict(model, x):
    out = model([x[:, i] for i in range(x.shape[1])])
    return np.broadcast_to(np.asarray(out, dtype=np.float64), (x.shape[0],)).copy()


def skill_from_pred(pred, theta, gamma, n, H, stride=1, tile=None):
    """(H, 9) from predictions pred (W_b or more, H, 2) on the first n rows of theta, gamma."""
    theta, gamma = np.asarray(theta, dtype=np.float64), np.asarray(gamma, dtype=np.float64)
    Wb = n_windows(n, H, stride)
    out = np.full((H, 9), np.nan)
    out[:, 4] = 0.0
    if Wb == 0:
        return out
    s = np.arange(Wb) * stride
    p = np.asarray(pred, dtype=np.float64)[:Wb]
    ok = np.ones(Wb, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(1, H + 1):
            ok = ok & np.isfinite(p[:, j - 1, 0]) & np.isfinite(p[:, j - 1, 1])
            yt, yg = theta[s + j], gamma[s + j]
            cnt = ok & np.isfinite(yt) & np.isfinite(yg)
            et, eg, ht, hg = p[:, j - 1, 0] - yt, p[:, j - 1, 1] - yg, theta[s] - yt, gamma[s] - yg
            z = lambda v: np.where(cnt, v, 0.0)
            n_ok = law_sum(z(np.ones(Wb)), tile)
            if n_ok == 0:
                continue
            ss_t, ss_g = law_sum(z(et * et), tile), law_sum(z(eg * eg), tile)
            out[j - 1] = (np.sqrt(np.float64(ss_t) / n_ok), np.sqrt(np.float64(ss_g) / n_ok), np.max(np.abs(et[cnt])),
                          np.max(np.abs(eg[cnt])), n_ok, ss_t, ss_g, law_sum(z(ht * ht), tile), law_sum(z(hg * hg), tile))
    return out


def horizon_np(text_t, text_g, X, time, theta, gamma, mean, scale, H, stride=1, integrator=RK4, prev_mode=PREV_INTERP, slots=GEN1,
               n=None, tile=None, mutant=None):
    """(skill (H, 9), pred (W_b, H, 2)) of one pair on one recording, line for line the law of include/rovmpc.h.  `mutant`: a
    deliberately wrong variant for the tests of the bound -- "k3_state" evaluates k3 at k2's stage state, "prev_unshifted"
    never moves the previous node."""
    X, time = np.asarray(X, dtype=np.float64), np.asarray(time, dtype=np.float64)
    theta, gamma = np.asarray(theta, dtype=np.float64), np.asarray(gamma, dtype=np.float64)
    mean, scale = np.asarray(mean, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    T, F = X.shape
    n = T if n is None else int(n)
    s_th, s_ga, s_thp, s_gap, s_cos, s_sin = slots
    ft, fg = _model(text_t, F), _model(text_g, F)
    Wb = n_windows(n, H, stride)
    pred = np.full((Wb, H, 2), np.nan)
    if Wb == 0:
        return skill_from_pred(pred, theta, gamma, n, H, stride, tile), pred
    s = np.arange(Wb) * stride                                              # windows
    th, ga = theta[s].copy(), gamma[s].copy()                                # state at node i = s
    thm, gam = theta[np.maximum(s - 1, 0)].copy(), gamma[np.maximum(s - 1, 0)].copy()      # the previous node
    scaled = lambda y, k: (y - mean[k]) / scale[k]
    with np.errstate(all="ignore"):
        for j in range(1, H + 1):                                           # step: row i - 1 -> row i = s + j
            i = s + j
            dt = time[i] - time[i - 1]

            def stage(yth, yga, c):
                x = X[i - 1].copy() if c == 0 else (X[i].copy() if c == 1 else (X[i - 1] + X[i]) / 2)
                x[:, s_th], x[:, s_ga] = scaled(yth, s_th), scaled(yga, s_ga)
                if s_cos >= 0:
                    x[:, s_cos] = scaled(np.cos(yth), s_cos)
                if s_sin >= 0:
                    x[:, s_sin] = scaled(np.sin(yga), s_sin)
                for slot, ym, y in ((s_thp, thm, th), (s_gap, gam, ga)):
                    if slot >= 0:
                        a, b = scaled(ym, slot), scaled(y, slot)
                        x[:, slot] = a if (prev_mode == PREV_HOLD or c == 0) else (b if c == 1 else (a + b) / 2)
                return _predict(ft, x), _predict(fg, x)

            k1 = stage(th, ga, 0)
            if integrator == EULER:
                th_n, ga_n = th + k1[0] * dt, ga + k1[1] * dt
            else:
                k2 = stage(th + (dt / 2) * k1[0], ga + (dt / 2) * k1[1], 0.5)
                kk = k1 if mutant == "k3_state" else k2
                k3 = stage(th + (dt / 2) * kk[0], ga + (dt / 2) * kk[1], 0.5)
                k4 = stage(th + dt * k3[0], ga + dt * k3[1], 1)
                th_n = th + (dt / 6) * (((k1[0] + 2 * k2[0]) + 2 * k3[0]) + k4[0])
                ga_n = ga + (dt / 6) * (((k1[1] + 2 * k2[1]) + 2 * k3[1]) + k4[1])
            if mutant != "prev_unshifted":
                thm, gam = th, ga
            th, ga = th_n, ga_n
            pred[:, j - 1, 0], pred[:, j - 1, 1] = th, ga
    return skill_from_pred(pred, theta, gamma, n, H, stride, tile), pred


def column_bounds(skill_ref, n_max):
    """Allowed |difference| of columns 0-3 from skill_from_pred on the same pred bits: rmse is a division and a square root of
    identical sums (2 roundings each side, doubled: 4 u relative); the maxima are maxima of identical differences: 0."""
    b = np.zeros_like(skill_ref)
    b[:, 0:2] = np.nan_to_num(4 * U * np.abs(skill_ref[:, 0:2]))          # (a NaN column must be NaN on both sides: the caller's check)
    return b


# ---- 50 digits ------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _evaluator(text):
    return SlotEvaluator(text, er.F64)


def horizon_true(text_t, text_g, X, time, theta, gamma, mean, scale, H, starts, integrator=RK4, prev_mode=PREV_INTERP, slots=GEN1):
    """For each start row s of `starts`: a list over j = 1 .. H of (theta*, gamma*, S_theta, S_gamma) at 50 digits, S the
    entry's scale; the list ends at the first step that leaves an operation's domain or the finite range."""
    X = np.asarray(X, dtype=np.float64)
    F = X.shape[1]
    s_th, s_ga, s_thp, s_gap, s_cos, s_sin = slots
    ft, fg = _evaluator(text_t), _evaluator(text_g)
    m = lambda v: mpf(float(v))
    zero = [0.0] * F
    out = []
    with mp.workdps(DPS):
        mu, sc = [m(v) for v in mean], [m(v) for v in scale]
        scaled = lambda y, k: (y - mu[k]) / sc[k]
        for s in starts:
            th, ga = m(theta[s]), m(gamma[s])
            thm, gam = m(theta[max(s - 1, 0)]), m(gamma[max(s - 1, 0)])
            S_t, S_g = abs(th), abs(ga)
            steps = []
            for j in range(1, H + 1):
                i = s + j
                dt = m(time[i]) - m(time[i - 1])
                x0, x1 = [m(v) if np.isfinite(v) else None for v in X[i - 1]], [m(v) if np.isfinite(v) else None for v in X[i]]

                def stage(yth, yga, c):
                    if c == 0:
                        x = list(x0)
                    elif c == 2:
                        x = list(x1)
                    else:
                        x = [None if a is None or b is None else (a + b) / 2 for a, b in zip(x0, x1)]
                    x[s_th], x[s_ga] = scaled(yth, s_th), scaled(yga, s_ga)
                    if s_cos >= 0:
                        x[s_cos] = scaled(mp.cos(yth), s_cos)
                    if s_sin >= 0:
                        x[s_sin] = scaled(mp.sin(yga), s_sin)
                    for slot, ym, y in ((s_thp, thm, th), (s_gap, gam, ga)):
                        if slot >= 0:
                            a, b = scaled(ym, slot), scaled(y, slot)
                            x[slot] = a if (prev_mode == PREV_HOLD or c == 0) else (b if c == 2 else (a + b) / 2)
                    kt, _ = ft(x, zero)
                    kg, _ = fg(x, zero)
                    return None if kt is None or kg is None else (kt, kg)

                k1 = stage(th, ga, 0)
                if k1 is None:
                    break
                if integrator == EULER:
                    th_n, ga_n = th + k1[0] * dt, ga + k1[1] * dt
                else:
                    k2 = stage(th + dt / 2 * k1[0], ga + dt / 2 * k1[1], 1)
                    k3 = k2 and stage(th + dt / 2 * k2[0], ga + dt / 2 * k2[1], 1)
                    k4 = k3 and stage(th + dt * k3[0], ga + dt * k3[1], 2)
                    if not k4:
                        break
                    th_n = th + dt / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0])
                    ga_n = ga + dt / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1])
                if abs(th_n) > er.F64.max or abs(ga_n) > er.F64.max:
                    break
                S_t, S_g = S_t + abs(th_n - th), S_g + abs(ga_n - ga)
                thm, gam, th, ga = th, ga, th_n, ga_n
                steps.append((th, ga, S_t, S_g))
            out.append(steps)
    return out


def value_errors(pred, true, starts, stride, pred_np=None):
    """Largest |got - exact| / (u S) of pred (W, H, 2) over the windows `starts`; where the 50-digit run stopped, the entry
    must be finite exactly where pred_np is (or non-finite when no pred_np is given) -- a miss there gives inf."""
    worst = 0.0
    with mp.workdps(DPS):
        for s, steps in zip(starts, true):
            w = s // stride
            for j in range(pred.shape[1]):
                got = pred[w, j]
                if j < len(steps):
                    for c in (0, 1):
                        if not np.isfinite(got[c]):
                            return np.inf
                        worst = max(worst, float(abs(mpf(float(got[c])) - steps[j][c]) / (U * steps[j][2 + c])))
                else:
                    want = np.isfinite(pred_np[w, j]) if pred_np is not None else np.array([False, False])
                    if (np.isfinite(got) != want).any():
                        return np.inf
    return worst


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
class Fixture:
    """One call of score_pairs: two fronts, the pairs, recordings (B, T, ...) with their lengths, the scaler, the parameters."""

    def __init__(self, name, theta_rows, gamma_rows, pairs, X, time, theta, gamma, mean, scale, H, stride=1, integrator=RK4,
                 prev_mode=PREV_INTERP, slots=GEN1, lengths=None, chosen=None):
        self.name, self.theta_rows, self.gamma_rows, self.pairs = name, list(theta_rows), list(gamma_rows), [tuple(p) for p in pairs]
        self.X, self.time, self.theta, self.gamma = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, time, theta, gamma))
        self.mean, self.scale, self.H, self.stride, self.integrator, self.prev_mode, self.slots = mean, scale, H, stride, integrator, prev_mode, slots
        self.lengths = [self.X.shape[1]] * self.X.shape[0] if lengths is None else list(lengths)
        self.chosen = chosen

    def np_pair(self, q, b, mutant=None):
        return _np_pair(self, q, b, mutant)

    def checked(self, q, b):
        """The (pair, recording)'s start rows that horizon_true is run on: the first, the last, the tile's edges, a few between."""
        Wb = n_windows(self.lengths[b], self.H, self.stride)
        ws = sorted({w for w in (0, 1, Wb // 3, TILE - 1, TILE, Wb - 2, Wb - 1) if 0 <= w < Wb})
        return [w * self.stride for w in ws]

    def true_pair(self, q, b):
        return _true_pair(self, q, b)

    def kwargs(self):
        """The keyword arguments of scoring.score_pairs for this fixture."""
        names = ("theta", "gamma", "theta_prev", "gamma_prev", "cos_theta", "sin_gamma")
        return dict(horizon=self.H, stride=self.stride, pairs=self.pairs, integrator="rk4" if self.integrator == RK4 else "euler",
                    prev_mode="interp" if self.prev_mode == PREV_INTERP else "hold",
                    feature_map={k: v for k, v in zip(names, self.slots) if v >= 0}, lengths=self.lengths)


@lru_cache(maxsize=None)
def _np_pair(fx, q, b, mutant):
    it, ig = fx.pairs[q]
    return horizon_np(fx.theta_rows[it], fx.gamma_rows[ig], fx.X[b], fx.time[b], fx.theta[b], fx.gamma[b], fx.mean, fx.scale, fx.H, fx.stride,
                      fx.integrator, fx.prev_mode, fx.slots, n=fx.lengths[b], mutant=mutant)


@lru_cache(maxsize=None)
def _true_pair(fx, q, b):
    it, ig = fx.pairs[q]
    return horizon_true(fx.theta_rows[it], fx.gamma_rows[ig], fx.X[b], fx.time[b], fx.theta[b], fx.gamma[b], fx.mean, fx.scale, fx.H,
                        fx.checked(q, b), fx.integrator, fx.prev_mode, fx.slots)


def scaler():
    s = json.load(open(os.path.join(GOLDEN, "scaler.json")))
    return np.array(s["mean"], dtype=np.float64), np.array(s["scale"], dtype=np.float64)


@lru_cache(maxsize=None)
def fixture_a():
    """The recorded replay table (T = 200, F = 18, non-uniform time) with all 23 x 14 generation-1 pairs.  Truth = horizon_np's
    single window (s = 0, H = 199) of the reference's chosen pair from (theta0, gamma0) plus 1e-3 std N(0, 1) noise
    (default_rng(1) for each series), written into the rows' own state slots as well.  H = 8, stride 1: 192 windows, one full
    tile and a ragged one."""
    d = np.load(os.path.join(GOLDEN, "kat_replay.npz"))
    eqs = json.load(open(os.path.join(GOLDEN, "equations.json")))
    fronts, chosen = [], []
    for key in ("dtheta_dt", "dgamma_dt"):
        rows = eqs[key]["rows"]
        fronts.append([r["sympy_format"] for r in rows])
        chosen.append([r["complexity"] for r in rows].index(eqs[key]["chosen_complexity"]))
    mean, scale = scaler()
    X, time = np.ascontiguousarray(d["Xs"], dtype=np.float64), np.ascontiguousarray(d["time"], dtype=np.float64)
    T = len(time)
    start_t, start_g = np.full(T, float(d["theta0"])), np.full(T, float(d["gamma0"]))
    _, clean = horizon_np(fronts[0][chosen[0]], fronts[1][chosen[1]], X, time, start_t, start_g, mean, scale, T - 1)
    series = []
    for c, y0 in ((0, start_t[0]), (1, start_g[0])):
        y = np.concatenate([[y0], clean[0, :, c]])
        series.append(y + 1e-3 * np.std(y) * np.random.default_rng(1).standard_normal(T))
    # the state slots of the rows hold the truths, as extract_features writes a recording (rovmpc_score_pairs never reads them;
    # the open-loop ranking of select_model does)
    X = X.copy()
    for slot, y in ((14, series[0]), (15, series[1]), (16, np.concatenate([series[0][:1], series[0][:-1]])),
                    (17, np.concatenate([series[1][:1], series[1][:-1]]))):
        X[:, slot] = (y - mean[slot]) / scale[slot]
    pairs = [(it, ig) for it in range(len(fronts[0])) for ig in range(len(fronts[1]))]
    return Fixture("A", fronts[0], fronts[1], pairs, X[None], time[None], series[0][None], series[1][None], mean, scale, 8,
                   chosen=pairs.index((chosen[0], chosen[1])))


A_TRUE_PAIRS = 23                        # fixture A's 50-digit runs: pair (it, it % 14) for every theta row, so every row is in one


def a_true_pairs():
    fx = fixture_a()
    return [fx.pairs.index((it, it % len(fx.gamma_rows))) for it in range(A_TRUE_PAIRS)] + [fx.chosen]


B_LENGTHS = lambda H: (1, 2, H, H + 1, TILE + H, 2 * TILE + H + 3)
B_PAIRS = ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 0), (3, 1), (1, 3))


@lru_cache(maxsize=None)
def fixture_b(H, stride, integrator=RK4, prev_mode=PREV_INTERP, gen2=False):
    """Synthetic scaled rows N(0, 1), time = cumsum U(0.005, 0.03), slow random-walk truths, one ragged batch of the lengths
    B_LENGTHS(H).  Rows: a state-difference row, the reference's chosen row, the deepest stack, and log(x3), non-finite on
    about half the rows.  gen2: F = 17 with the generation-2 slots (theta, gamma at 12, 13; cos theta, sin gamma at 14, 15)."""
    fa = fixture_a()
    F = 17 if gen2 else 18
    lengths = B_LENGTHS(H)
    T, B = max(lengths), len(lengths)
    rng = np.random.default_rng(9000 + 100 * H + 10 * stride + gen2)
    X = rng.standard_normal((B, T, F))
    time = np.cumsum(rng.uniform(0.005, 0.03, (B, T)), axis=1)
    theta = 0.3 + np.cumsum(0.01 * rng.standard_normal((B, T)), axis=1)
    gamma = -0.2 + np.cumsum(0.01 * rng.standard_normal((B, T)), axis=1)
    mean, scale = 0.1 * rng.standard_normal(F), rng.uniform(0.5, 2.0, F)
    if gen2:
        theta_rows = ("x12 - x15", "0.3*x14*x13 - x16", er.deep_expression(), "log(x3)")
        gamma_rows = ("x14 - x13", "sin(x12) - 0.5*x15", er.deep_expression(), "log(x3)")
    else:
        it, ig = fa.pairs[fa.chosen]
        theta_rows = ("x15 - x17", fa.theta_rows[it], er.deep_expression(), "log(x3)")
        gamma_rows = ("x14 - x16", fa.gamma_rows[ig], er.deep_expression(), "log(x3)")
    return Fixture("B(H=%d,stride=%d,%s,%s,%s)" % (H, stride, "rk4" if integrator == RK4 else "euler", "interp" if prev_mode == PREV_INTERP else "hold",
                                                   "gen2" if gen2 else "gen1"),
                   theta_rows, gamma_rows, B_PAIRS, X, time, theta, gamma, mean, scale, H, stride, integrator, prev_mode, GEN2 if gen2 else GEN1, lengths)


def b_fixtures():
    """H in {1, 5} x stride in {1, 3}; both prev modes and both integrators; the generation-2 variant."""
    out = [fixture_b(H, stride) for H in (1, 5) for stride in (1, 3)]
    out += [fixture_b(5, 1, RK4, PREV_HOLD), fixture_b(5, 3, EULER, PREV_INTERP), fixture_b(5, 1, EULER, PREV_HOLD)]
    out += [fixture_b(5, 1, RK4, PREV_INTERP, True), fixture_b(5, 3, EULER, PREV_INTERP, True)]
    return out


def checked_cases():
    """(fixture, pair, recording) of every 50-digit run."""
    cases = [(fixture_a(), q, 0) for q in a_true_pairs()]
    for fx in b_fixtures():
        cases += [(fx, q, b) for q in range(len(fx.pairs)) for b in range(len(fx.lengths)) if n_windows(fx.lengths[b], fx.H, fx.stride) > 0]
    return cases


def measure(pred_of, mutant=None):
    """Largest error figure over checked_cases() of pred_of(fixture, q, b) -> pred (W, H, 2), and where."""
    worst, where = 0.0, None
    for fx, q, b in checked_cases():
        e = value_errors(pred_of(fx, q, b), fx.true_pair(q, b), fx.checked(q, b), fx.stride, fx.np_pair(q, b)[1])
        if e > worst:
            worst, where = e, (fx.name, q, b)
    return worst, where
