"""The second-order (generation-3, features_dd) rollout of oracle.rollout_vec_dd at 50 digits, with a bound on the error that
float arithmetic of type T may accumulate over the horizon, and the deterministic workspace the kernels are held to.

Why not step by step.  tests/rollout_reference.py restarts every step from the tested side's own nodes.  Here the step map
carries more than the returned (theta_n, gamma_n): the rates (dtheta_n, dgamma_n) and, with the composed velocity transform, the
velocity and the surge / sway speeds that the next node differences against.  None of it is returned, so the comparison is
GLOBAL: the whole exact trajectory against the whole returned one, with a first-order bound propagated along it.

The law.  y = (theta, gamma, dtheta, dgamma), y' = (dtheta, dgamma, f_theta(x), f_gamma(x)); classic RK4 with the rows of nodes
n and n + 1 averaged at the two midpoint stages, or the reference's explicit double Euler.  Row x: slots 0..3 the scaled stage
state, slots 4..13 the scaled [v_sway, v_surge, a_sway, a_surge, V(3), A(3)] with unit = rel / (|rel| + 1e-8), W = v_scale V (m/s),
v_surge = W . unit, v_sway = |W x unit|, a_sway / a_surge the first differences to the previous node (node 0: the first
difference of nodes 0 and 1, np.gradient's edge rule), A_n = (V_n - V_{n-1}) / h scaled by v_scale, A_0 from the state.  P and V as
in rollout_reference (Rollout.P, Rollout.V, _rot: reused).  The state, the controls, the scaler, the configuration and the
rotation table are exact after one rounding to T; the constants of the model's text are rounded as expr_reference.Evaluator
rounds them.  Slopes: rollout_reference.SlotEvaluator on the model's text with the 14 variable names mapped to x0..x13.

Carried state z_n.  Without the composed transform every exogenous slot is a function of the inputs alone: z = y, 4 entries.
With it V_{n+1} is U_n rotated by (theta_n, gamma_n), and the row of node n reads V_n, the speeds of node n and their
differences to node n - 1, so the map z_n -> z_{n+1} closes on 14 entries: y, V(3), v_sway, v_surge, a_sway, a_surge, A(3).
(Nine -- y, V and the two speeds -- do not close the map: the differences of node n read node n - 1.)

Bound.  E_0 holds the creation error of the node-0 entries the kernel computes (the two speeds and their edge-rule differences;
zero for y, V, A), and E_{n+1} = |Phi_n| E_n + u_n with
  u_n      the local scale of step n per entry of z, built as rollout_reference builds scale_th: for y
           eps (|y_n| + |y*|) + c sum_j |b_j| eps |k_j*| + c sum_j |b_j| B_j, B_j the evaluator's running bound of stage j's slope
           (for theta and gamma, whose slopes are the stage rates: the rate's own stage uncertainty).  Slot uncertainties count
           (number of roundings) x (sum of the absolute terms):  W = v_scale V: v_scale e_V + eps/2 |W|;  unit: as
           rollout_reference's, reciprocal and product counted;  v_surge: sum (|W_i| e_unit_i + |unit_i| e_W_i) + 2 eps sum |W_i unit_i|;
           v_sway: the 2-norm of the cross product's component errors (each 3/2 eps of its two products and the four first-order
           terms) + 2 eps v_sway (squares, sum, root);  a_sway, a_surge, A: (e_n + e_m) / h + (3/2) eps (|s_n| + |s_m|) / h;  scaling
           2 eps (|raw| + |mean|) / scale;  midpoint: the mean of the two uncertainties + eps/2 of the mean magnitude.
           Composed transform: the raw entries of row n are z's own (their error is E_n, carried by Phi), only their scaling is
           local; the entries of row n + 1 are created in step n: their creation error enters the stages that read them AND u_n.
  |Phi_n|  the Jacobian of the exact step map at z*_n by central differences (relative perturbation 1e-25 at 60 digits),
           entries in absolute value.  The column of an exogenous entry has no y part where neither expression reads its slot of
           row n or the slot of row n + 1 that differences against it.
Compared: |theta_n - theta*_n| <= M_DD E_n[theta], |gamma_n - gamma*_n| <= M_DD E_n[gamma], n = 1..N.  N = 1 is the purely local check.

Undecided -- not compared, by the reference and the inputs alone: (a) E_n above UND_KAPPA = 1e-3 of the path length
sum_{m<n} |theta*_{m+1} - theta*_m| (gamma likewise); (b) composed transform: an axis branch (n_xy, n_th < 1e-9) of a node
before n within its own budget of the threshold; (c) a slope outside T's range or an operation's domain from the step on where
it happens -- a divisor within its own uncertainty of zero is one --, or an input that is not finite (NaN nodes are compared as
NaN by the tests).

Margin.  M_DD is twice the largest ratio, over table_dd(8) in fp64 (default rows, the composed transform, RK4), of the float64
oracle's own error |rollout_vec_dd node - z*| to E_n, never below 4; fp32 uses the same M_DD with eps32.
tests/test_rollout_dd_reference_host.py measures it again and fails if the oracle leaves M_DD / 2."""
import ast
import collections
import functools
import json
import math
import os
import re

import mpmath as mp
import numpy as np
from mpmath import mpf

import cable_reference as cr
import expr_reference as er
import rollout_reference as rr

DPS = rr.DPS
M_DD = 4.0                      # measured: largest ratio of the float64 oracle 0.204 (theta), 0.211 (gamma); 2 x 0.211 < 4
UND_KAPPA = rr.UND_KAPPA
REL_STEP = mpf(10) ** -25       # central differences of the step map
NAMES = ("theta", "gama", "dtheta", "dgamma", "v_sway", "v_surge", "a_sway", "a_surge", "V_x", "V_y", "V_z", "a_x", "a_y", "a_z")
C_RCP = {"f64": 1.0, "f32": 2.0}                # the reciprocal behind unit
# entry of z (composed transform) -> slot of the row that reads it
Z_SLOT = {4: 8, 5: 9, 6: 10, 7: 4, 8: 5, 9: 6, 10: 7, 11: 11, 12: 12, 13: 13}
# ... -> slot of row n + 1 that differences against it (V -> A, the speeds -> their first differences)
Z_DIFF = {4: 11, 5: 12, 6: 13, 7: 6, 8: 7}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TrajRef = collections.namedtuple("TrajRef", "th ga E_th E_ga und_th und_ga")


# ---- the model ---------------------------------------------------------------------------------------------------------------
def slot_text(text, names=NAMES):
    """The model's text with the variable names mapped to x0..x13."""
    idx = {n: i for i, n in enumerate(names)}
    return re.sub(r"\b(%s)\b" % "|".join(sorted(names, key=len, reverse=True)), lambda m: "x%d" % idx[m.group(1)], text)


def texts_of(model):
    """(f_theta, f_gamma) texts of a product model (expr_theta / expr_gamma) or an oracle model (f_theta.expr / f_gamma.expr)."""
    if hasattr(model, "expr_theta"):
        return model.expr_theta, model.expr_gamma
    return model.f_theta.expr, model.f_gamma.expr


@functools.lru_cache(maxsize=None)
def oracle_model_dd(ct=None, cg=None):
    """The oracle's model of Pareto rows (ct, cg) of the second-order run (default: the chosen rows, 6 / 5) with that run's scaler."""
    from oracle import rovmpc_oracle as orc
    eq = json.load(open(os.path.join(GOLDEN, "equations_gen3.json")))
    sc = json.load(open(os.path.join(GOLDEN, "scaler_gen3.json")))

    def row(which, c):
        c = c or eq[which]["chosen_complexity"]
        return [r for r in eq[which]["rows"] if r["complexity"] == c][0]["sympy_format"]
    names = eq["variable_names"]
    return orc.DynamicsModel(np.array(sc["mean"]), np.array(sc["scale"]), orc.SymbolicModel(row("ddtheta", ct), 14, names),
                             orc.SymbolicModel(row("ddgamma", cg), 14, names))


class DDEvaluator(rr.SlotEvaluator):
    """SlotEvaluator whose quotient is undefined where the divisor lies within its own uncertainty of zero (the first-order
    bound says nothing there)."""

    def _ev(self, node):
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Div):
            b, eb = self._ev(node.right)
            if abs(b) <= eb:
                raise er._Undefined
        return super()._ev(node)


@functools.lru_cache(maxsize=None)
def _evaluator(text, fmt):
    return DDEvaluator(slot_text(text), er.FMT[fmt])


def _slots_read(text):
    return {int(s) for s in re.findall(r"\bx(\d+)\b", slot_text(text))}


# ---- one candidate -------------------------------------------------------------------------------------------------------------
class RolloutDD(rr.Rollout):
    """One candidate's exact second-order trajectory with its propagated bound.  `mutate`: a law broken in one place, for the
    host test alone ("weights": b_2 = 2 + 1e-7; "midpoint": the row of node n at the half stages; "edge": node 0's first
    difference on nodes 0 and 2)."""

    def __init__(self, cfg, model, state, U_k, fmt="f64", Rtab=None):
        U_k = np.asarray(U_k, dtype=np.float64)
        tt, tg = texts_of(model)
        shim = collections.namedtuple("Shim", "mean scale f_theta f_gamma")(model.mean, model.scale, "0.0", "0.0")
        super().__init__(cfg, shim, state, U_k, np.zeros((len(U_k) + 1, 2)), fmt, Rtab)
        self.ft, self.fg = _evaluator(tt, fmt), _evaluator(tg, fmt)
        self.read = _slots_read(tt) | _slots_read(tg)
        self.compose = cfg.vt_mode == 1
        self.N = len(U_k)
        self._at = None
        self._unit, self._row, self._kin = {}, {}, {}
        st = np.asarray(state.as_array() if hasattr(state, "as_array") else state, dtype=np.float64)
        with mp.workdps(DPS):
            self.start = [self.r(st[12]), self.r(st[13])]

    # -- kinematics --------------------------------------------------------------------------------------------------------------
    def node(self, m):
        """Rollout.V's (theta, gamma) of node m: the pair the step map is evaluated at."""
        return self._at

    def vel(self, m, th=None, ga=None):
        """(V_m, 2-norm uncertainty) through Rollout.V; composed transform: U_{m-1} rotated by the given (theta, gamma) of node m - 1."""
        if self.compose and m > 0:
            self._at = (th, ga)
            self._V.pop(m, None)
        return self.V(m)

    def kin(self, m, th=None, ga=None):
        """(V_m, e_V, v_sway, v_surge, e_sway, e_surge, W, e_W) of node m, None where V_m is undefined; kept per (m, theta, gamma)."""
        key = (m, th, ga) if self.compose and m > 0 else m
        if key not in self._kin:
            V, eV = self.vel(m, th, ga)
            self._kin[key] = None if V is None else (V, eV) + self.speeds(V, eV, m)
        return self._kin[key]

    def unit(self, m):
        """(unit_m, per-component uncertainty): rel / (|rel| + 1e-8)."""
        if m not in self._unit:
            eps = self.F.eps
            P, eP = self.P(m)
            rel = [P[i] - self.P0[i] for i in range(3)]
            e_rel = [eP[i] + 0.5 * eps * float(abs(rel[i])) for i in range(3)]
            nr = cr._norm(rel)
            e_nr = (sum(float(abs(rel[i])) * e_rel[i] for i in range(3)) / float(nr) if nr > 0 else sum(e_rel)) + 2 * eps * float(nr)
            d = nr + self.c8
            u = [rel[i] / d for i in range(3)]
            own = (C_RCP[self.F.name] + 0.5) * eps
            e_u = [float(e_rel[i] / d + abs(u[i]) / d * (e_nr + 0.5 * eps * float(d))) + own * float(abs(u[i])) for i in range(3)]
            self._unit[m] = (u, e_u)
        return self._unit[m]

    def speeds(self, V, eV, m):
        """(v_sway, v_surge, e_sway, e_surge, W, e_W) of the velocity V (2-norm uncertainty eV) at node m; W = v_scale V."""
        eps = self.F.eps
        u, eu = self.unit(m)
        W = [self.vs * x for x in V]
        eW = [float(abs(self.vs)) * eV + 0.5 * eps * float(abs(w)) for w in W]
        surge = sum((W[i] * u[i] for i in range(3)), mpf(0))
        mag = float(sum((abs(W[i] * u[i]) for i in range(3)), mpf(0)))
        e_surge = sum(float(abs(W[i])) * eu[i] + float(abs(u[i])) * eW[i] for i in range(3)) + 2 * eps * mag
        c, e_c = [], []
        for i, j in ((1, 2), (2, 0), (0, 1)):
            c.append(W[i] * u[j] - W[j] * u[i])
            e_c.append(float(abs(W[i])) * eu[j] + float(abs(u[j])) * eW[i] + float(abs(W[j])) * eu[i] + float(abs(u[i])) * eW[j]
                       + 1.5 * eps * float(abs(W[i] * u[j]) + abs(W[j] * u[i])))
        sway = cr._norm(c)
        e_sway = math.sqrt(sum(x * x for x in e_c)) + 2 * eps * float(sway)
        return sway, surge, e_sway, e_surge, W, eW

    def _diff(self, a, ea, b, eb):
        """((a - b) / h, its uncertainty)."""
        return (a - b) / self.h, float((ea + eb + 1.5 * self.F.eps * (abs(a) + abs(b))) / self.h)

    def _scale_row(self, raw, e_raw):
        vals = [(raw[p] - self.mean[4 + p]) / self.scale[4 + p] for p in range(10)]
        errs = [self._scaled(raw[p], e_raw[p], 4 + p) for p in range(10)]
        return vals, errs

    def _acc(self, A, eA):
        """(v_scale A, uncertainty) per component."""
        out = [self.vs * a for a in A]
        return out, [float(abs(self.vs)) * e + 0.5 * self.F.eps * float(abs(o)) for e, o in zip(eA, out)]

    def exo_row(self, m, edge=1):
        """The scaled row of node m where it hangs on the inputs alone (no composed transform): (values, uncertainties) of the
        slots 4..13, or None where a value is undefined.  `edge`: the neighbour of node 0's first difference."""
        if m in self._row:
            return self._row[m]
        nb = edge if m == 0 else m - 1
        if nb > self.N:
            nb = m                                              # (a mutant's neighbour beyond the horizon: no difference)
        ka, kb = self.kin(m), self.kin(nb)
        if ka is None or kb is None:
            self._row[m] = None
            return None
        V, eV, sw, su, e_sw, e_su, W, eW = ka
        Vn, eVn, swn, sun, e_swn, e_sun, _, _ = kb
        sgn = -1 if m == 0 else 1
        a_sw, e_asw = self._diff(sw, e_sw, swn, e_swn)
        a_su, e_asu = self._diff(su, e_su, sun, e_sun)
        if m == 0:
            A, eA = self.A1, [0.0] * 3
            if nb != 1:                                          # (mutant: the difference of nodes 0 and `edge` over their distance)
                a_sw, a_su = a_sw / nb, a_su / nb
        else:
            A, eA = zip(*[self._diff(V[i], eV, Vn[i], eVn) for i in range(3)])
        A, eA = self._acc(A, eA)
        self._row[m] = self._scale_row([sw, su, sgn * a_sw, sgn * a_su] + W + list(A), [e_sw, e_su, e_asw, e_asu] + eW + list(eA))
        return self._row[m]

    # -- the step map --------------------------------------------------------------------------------------------------------------
    def z0(self):
        """(z_0, E_0): see the module text."""
        y = list(self.start) + list(self.prev)
        if not self.compose:
            return y, [0.0] * 4
        k1 = self.kin(1, y[0], y[1])
        if k1 is None:
            return None, None
        _, _, sw, su, e_sw, e_su, _, _ = self.kin(0)
        _, _, sw1, su1, e_sw1, e_su1, _, _ = k1
        a_sw, e_asw = self._diff(sw1, e_sw1, sw, e_sw)
        a_su, e_asu = self._diff(su1, e_su1, su, e_su)
        return y + list(self.V1) + [sw, su, a_sw, a_su] + list(self.A1), [0.0] * 7 + [e_sw, e_su, e_asw, e_asu] + [0.0] * 3

    def step(self, n, z, rk=True, mutate=None):
        """(z_{n+1}, u_n) of the exact step map at z, None where undefined; rk=False: the exogenous entries alone (y part None)."""
        with mp.workdps(DPS + 10):
            return self._step_dd(n, z, rk, mutate)

    def _step_dd(self, n, z, rk, mutate):
        eps = self.F.eps
        y = list(z[:4])
        if not self.compose:
            xa, xb = self.exo_row(n, 2 if mutate == "edge" else 1), self.exo_row(n + 1)
            if xa is None or xb is None:
                return None
            return self._rk(y, xa, xb, mutate)
        kn = self.kin(n + 1, y[0], y[1])
        if kn is None:
            return None
        V, eV, sw, su, e_sw, e_su, W, eW = kn
        a_sw, e_asw = self._diff(sw, e_sw, z[7], 0.0)
        a_su, e_asu = self._diff(su, e_su, z[8], 0.0)
        A, eA = zip(*[self._diff(V[i], eV, z[4 + i], 0.0) for i in range(3)])
        exo = list(V) + [sw, su, a_sw, a_su] + list(A)
        u_exo = [eV] * 3 + [e_sw, e_su, e_asw, e_asu] + list(eA)
        if not rk:
            return [None] * 4 + exo, None
        Wa = [self.vs * x for x in z[4:7]]
        Aa, eAa = self._acc(z[11:14], [0.0] * 3)
        xa = self._scale_row([z[7], z[8], z[9], z[10]] + Wa + Aa, [0.0] * 4 + [0.5 * eps * float(abs(w)) for w in Wa] + eAa)
        Ab, eAb = self._acc(A, eA)
        xb = self._scale_row([sw, su, a_sw, a_su] + W + Ab, [e_sw, e_su, e_asw, e_asu] + eW + eAb)
        out = self._rk(y, xa, xb, mutate)
        if out is None:
            return None
        return out[0] + exo, out[1] + u_exo

    def _rk(self, y, xa, xb, mutate=None):
        """(y_{n+1}, u of its four entries) from y and the scaled rows of the two nodes."""
        F, eps, h, cfg = self.F, self.F.eps, self.h, self.cfg
        mean, scale = self.mean, self.scale
        if mutate == "midpoint":
            xm = xa
        else:
            xm = ([(a + b) / 2 for a, b in zip(xa[0], xb[0])],
                  [(a + b) / 2 + 0.25 * eps * float(abs(u) + abs(v)) for a, b, u, v in zip(xa[1], xb[1], xa[0], xb[0])])

        def stage(s, es, c):
            exo = (xa, xm, xb)[c]
            vals = [(s[i] - mean[i]) / scale[i] for i in range(4)] + list(exo[0])
            errs = [self._scaled(s[i], es[i], i) for i in range(4)] + list(exo[1])
            kt, Bt = self.ft(vals, errs)
            kg, Bg = self.fg(vals, errs)
            if kt is None or kg is None:
                return None
            return (s[2], s[3], kt, kg), (es[2], es[3], Bt, Bg)

        k = [stage(y, [0.0] * 4, 0)]
        if k[0] is None:
            return None
        if cfg.integrator == 1:
            b, c = (1,), h
        else:
            b, c = ((1, 2 + mpf(10) ** -7, 2, 1) if mutate == "weights" else rr.B_RK4), h / 6
            for a, cc in ((mpf(1) / 2, 1), (mpf(1) / 2, 1), (mpf(1), 2)):
                kj, Bj = k[-1]
                s = [y[i] + a * h * kj[i] for i in range(4)]
                es = [eps * float(abs(s[i])) + float(a * h) * (eps * float(abs(kj[i])) + Bj[i]) for i in range(4)]
                k.append(stage(s, es, cc))
                if k[-1] is None:
                    return None
        yn = [y[i] + c * sum((bj * kj[0][i] for bj, kj in zip(b, k)), mpf(0)) for i in range(4)]
        cf = float(c)
        u = [eps * float(abs(y[i]) + abs(yn[i])) + cf * sum(bj * (eps * float(abs(kj[0][i])) + kj[1][i]) for bj, kj in zip(b, k))
             for i in range(4)]
        return yn, u

    def jacobian(self, n, z):
        """|Phi_n|: central differences of the step map at z, entries in absolute value (numpy, dim x dim)."""
        dim = len(z)
        Phi = np.zeros((dim, dim))
        with mp.workdps(DPS + 10):
            for i in range(dim):
                rk = i < 4 or Z_SLOT[i] in self.read or Z_DIFF.get(i) in self.read
                d = REL_STEP * (abs(z[i]) if z[i] != 0 else mpf(1))
                zp, zm = list(z), list(z)
                zp[i], zm[i] = z[i] + d, z[i] - d
                fp, fm = self.step(n, zp, rk), self.step(n, zm, rk)
                if fp is None or fm is None:
                    return None
                for j in range(dim):
                    if fp[0][j] is not None:
                        Phi[j, i] = float(abs(fp[0][j] - fm[0][j]) / (2 * d))
        return Phi

    # -- the trajectory ------------------------------------------------------------------------------------------------------------
    def trajectory(self, mutate=None, bound=True):
        """TrajRef over the nodes 0..N (entries of an undefined tail: None / inf / undecided)."""
        N = self.N
        th, ga = [None] * (N + 1), [None] * (N + 1)
        E_th, E_ga = np.full(N + 1, np.inf), np.full(N + 1, np.inf)
        und_th, und_ga = np.ones(N + 1, bool), np.ones(N + 1, bool)
        if not self.finite:
            return TrajRef(th, ga, E_th, E_ga, und_th, und_ga)
        with mp.workdps(DPS + 10):
            z, E = self.z0()
            if z is None:
                return TrajRef(th, ga, E_th, E_ga, und_th, und_ga)
            E = np.array(E)
            self.zs = [z]
            th[0], ga[0], E_th[0], E_ga[0] = z[0], z[1], 0.0, 0.0
            len_th = len_ga = 0.0
            for n in range(N):
                out = self.step(n, z, True, mutate)
                if out is None:
                    break
                if bound and E is not None:
                    Phi = self.jacobian(n, z)
                    E = None if Phi is None else Phi @ E + np.array(out[1])
                zn = out[0]
                len_th += float(abs(zn[0] - z[0])); len_ga += float(abs(zn[1] - z[1]))
                z = zn
                self.zs.append(z)
                th[n + 1], ga[n + 1] = z[0], z[1]
                if E is not None:
                    E_th[n + 1], E_ga[n + 1] = E[0], E[1]
                    close = self.compose and any(m in self.branch_close for m in range(n + 1))
                    und_th[n + 1] = close or not E[0] <= UND_KAPPA * len_th
                    und_ga[n + 1] = close or not E[1] <= UND_KAPPA * len_ga
        return TrajRef(th, ga, E_th, E_ga, und_th, und_ga)


_CACHE = {}


def trajectory_true(cfg, model, state, U, fmt="f64", Rtab=None):
    """One TrajRef per candidate.  Cached by the inputs (the reference never reads the tested side), so the parametrisations that
    share a case -- model paths, bit-identity checks, equal candidates -- compute it once."""
    state = np.asarray(state, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    base = (float(cfg.dt), float(cfg.v_scale), int(cfg.vt_mode), int(cfg.integrator), texts_of(model), np.asarray(model.mean).tobytes(),
            np.asarray(model.scale).tobytes(), state.tobytes(), fmt, None if Rtab is None else np.asarray(Rtab, dtype=np.float64).tobytes())
    out = []
    for k in range(len(U)):
        key = base + (U[k].tobytes(),)
        if key not in _CACHE:
            _CACHE[key] = RolloutDD(cfg, model, state, U[k], fmt, Rtab).trajectory()
        out.append(_CACHE[key])
    return out


def ratios(cfg, model, state, U, traj, fmt="f64", Rtab=None):
    """Per candidate and node 1..N: |node - reference| / E_n for theta and gamma (NaN where undecided, inf where a decided node
    is not finite)."""
    traj = np.asarray(traj, dtype=np.float64)
    refs = trajectory_true(cfg, model, state, U, fmt, Rtab)
    K, N = len(refs), traj.shape[1] - 1
    rt, rg = np.full((K, N), np.nan), np.full((K, N), np.nan)
    with mp.workdps(DPS):
        for k, ref in enumerate(refs):
            for n in range(1, N + 1):
                for col, want, E, und, out in ((0, ref.th, ref.E_th, ref.und_th, rt), (1, ref.ga, ref.E_ga, ref.und_ga, rg)):
                    if und[n]:
                        continue
                    got = float(traj[k, n, col])
                    if not math.isfinite(got):
                        out[k, n - 1] = np.inf
                    else:
                        err = float(abs(mpf(got) - want[n]))
                        out[k, n - 1] = err / E[n] if E[n] > 0 else (0.0 if err == 0 else np.inf)
    return rt, rg


worst = rr.worst


# ---- the deterministic workspace -----------------------------------------------------------------------------------------------
Row = rr.Row
RATES = ((0.013, -0.021), (0.0, 0.0), (0.5, -0.3), (-2.0, 1.5))
A_START = (5.0, -3.0, 2.0)
P0_OFF = (0.4, -0.3, 0.25)
VX0_ROW, BIG_ROW, NAN_ROW, NAN_CANDIDATE = 7, 3, 10, 6
K_TABLE = rr.K_TABLE
V_SCALE = 1e-3                  # MPCConfig's default: the controls and the state's velocity are in mm/s


def vx_of_scaled_zero():
    """V_x (mm/s) whose v_scale V_x is the float64 scaler mean of slot 8 exactly: the scaled V_x of node 0 is then an exact zero."""
    mean8 = oracle_model_dd().mean[8]
    v = mean8 / V_SCALE
    for _ in range(64):
        if V_SCALE * v == mean8:
            return float(v)
        v = np.nextafter(v, np.inf if V_SCALE * v < mean8 else -np.inf)
    raise ValueError("no float64 V_x with v_scale V_x == mean[8]")


def _state(op, rates, rel, V, P0=(0.0, 0.0, 0.0)):
    st = rr._state(op, 0.0, rel, V, P0)
    st[9:12] = A_START
    st[14:16] = rates
    return st


@functools.lru_cache(maxsize=None)
def table_dd(N=8, fmt="f64"):
    """The workspace: 10 state rows over the operating points 0, 2, 3, 4, 6 of rollout_reference.OPERATING, the four pairs of
    initial rates, the connection vectors and velocities of rollout_reference.table() and the velocity whose scaled V_x is
    an exact zero at node 0, each with rollout_reference.controls(); and the set with a NaN candidate.

    fp32 takes other inputs in two rows, where float arithmetic itself leaves less than half of the nodes decided (measured on
    the CPU, theta's share of the fp32 reference at N = 8):  row 1, rates (0, 0) at (0.6, -0.6): 0.000 -- theta moves 2e-5 over
    the horizon, 1e-3 of that is below eps32 |theta|; fp32 starts it from the rates (0.5, 0), which keeps a zero rate where it can
    be decided (theta 0.901, gamma 0.783).  Row 4, n_xy = 1e-3: 0.428 -- the theta axis is rel_xy / n_xy, its direction error
    eps32 |rel| / n_xy = 1e-4 per node; fp32 takes n_xy = 1e-2 (0.750)."""
    mean, _ = rr._scaler()
    rm, Vm = mean[0:3], mean[3:6]
    unit = rm / np.linalg.norm(rm)
    nxy = 1e-3 if fmt == "f64" else 1e-2
    rel = {"mean": rm, "+x": (1.2, 0.0, 0.0), "vertical": (0.0, 0.0, -1.4), "nxy": (nxy * 0.6, -nxy * 0.8, -1.1),
           "|rel|=1e-6": 1e-6 * unit, "|rel|=12": 12.0 * unit}
    vel = {"mean": Vm, "zero": np.zeros(3), "par": 50.0 * unit, "vx0": np.array([vx_of_scaled_zero(), Vm[1], Vm[2]])}
    still = (0.0, 0.0) if fmt == "f64" else (0.5, 0.0)
    spec = [(0, RATES[0], "mean", "mean", None), (2, still, "+x", "zero", None), (3, RATES[2], "vertical", "par", None),
            (4, RATES[3], "mean", "mean", None), (6, RATES[3], "nxy", "mean", P0_OFF), (0, RATES[2], "|rel|=1e-6", "zero", None),
            (2, RATES[3], "|rel|=12", "par", None), (3, RATES[2], "mean", "vx0", None), (4, RATES[2], "+x", "mean", P0_OFF),
            (6, RATES[3], "vertical", "mean", None)]
    rows = []
    for i, (op, rates, r, v, p0) in enumerate(spec):
        tag = "%d:(%g,%g) rates (%g,%g) rel=%s V=%s%s" % ((i,) + rr.OPERATING[op] + rates + (r if r != "nxy" else "nxy=%g" % nxy, v, " P0" if p0 else ""))
        rows.append(Row(tag, _state(op, rates, rel[r], vel[v], p0 or (0.0, 0.0, 0.0)), rr.controls(N, seed=200 + i)))
    U = rr.controls(N, seed=300)
    U[NAN_CANDIDATE] = np.nan
    rows.append(Row("nan:(-0.6,0.05) rates (0.5,-0.3) candidate 6 NaN", _state(3, RATES[2], rm, Vm), U))
    return tuple(rows)


SHAPES = ((1, 1), (1, 19), (2, 5), (7, 67), (12, 19))


def shape_case(N, K, fmt="f64"):
    """(state, U) of the shape tests: the (-2.0, 1.5) row, whose every step is a big one, with its own control seed."""
    return table_dd(N, fmt)[BIG_ROW].state, rr.controls(N, K, seed=200 + BIG_ROW)
