"""One step of the closed-loop rollout (oracle.rollout_vec, the step between two nodes of the (theta, gamma) trajectory) at 50
digits, the per-step error scale that ties a tolerance to the step's conditioning, the cost terms read off a returned
trajectory, and the deterministic workspace the kernels are held to.

The law.  `step_true(cfg, model, state, U_k, nodes, n)` restates the oracle's step n -> n + 1 for one candidate: P_n as the
exact sum P1 + (v_scale h) sum_{m<n} U_m; the velocity transform of U_{n-1} (vt_mode 0: itself; 1: R_theta(+theta) R_gamma(-gamma)
about the axes of P_{n-1} - P0, degenerate branches of the axes included; 2: the rotation table); A_n = (V_n - V_{n-1}) / h;
the exogenous feature rows of nodes n and n + 1 (generation-1 map: 14 scaled slots with the +1e-8 of the two norms, the
[1e-5, 10] clip of the tension and the [-1, 1] clip of angle_proj; generation-2 map: 12 unscaled slots and the unclipped
angle_proj); the delay slots (INTERP: node n - 1 at the start, node n at the end, their mean in between; HOLD: node n - 1);
classic RK4 with the feature rows averaged at the two midpoint stages, or explicit Euler.  `nodes` are the trajectory nodes the
side under test returned: the step starts from nodes[n] and reads nodes[n - 1] (delay slot, V_n) and nodes[n - 2] (V_{n-1} of
A_n) -- all taken as exact, like the state, the controls, the scaler and the configuration, each rounded to the type T under
test.  The reference therefore restarts from the tested side's own nodes in every step: the error compared is LOCAL, the
amplification of the chain (1e20 over twenty steps of 0.05 s in the gamma equation) cancels out.
Slopes are evaluated by expr_reference.Evaluator on the model's expression text.

Per-step scale.  With eps = 2^(1-p) of T, b = (1, 2, 2, 1), c = h / 6 (RK4) or b = (1), c = h (Euler), the scale of theta's step is

    u = eps (|theta_n| + |theta*|)  +  c sum_j |b_j| eps |k_j*|  +  c sum_j |b_j| B_j

(gamma likewise).  B_j is the Evaluator's running first-order bound of stage j's slope (every operation's own rounding, and
every slot's uncertainty carried through |df / d slot|).  A slot's uncertainty is built as estimation_reference.py builds its
sums: (number of roundings) x (sum of the absolute values of the terms that form the raw feature), the scaling
2 eps (|raw| + |mean|) / scale (subtraction, the reciprocal of the scale, the product), and for the stage's own state
eps |y_j| + a_j h E_{j-1}, E_{j-1} = eps |k*_{j-1}| + B_{j-1} the bound of the previous stage's slope.  The raw features:
  P_n        (n + 3) / 2 roundings of |P1| + v_scale h sum |U_m|   (a sequential sum of n terms, the product v_scale h)
  V_{n+1}    vt 0: exact.  vt 2: 5/2 roundings of sum_j |R_ij U_j|.  vt 1, per rotation, in the 2-norm:
             |v| [ dk (|s| + 2 |1 - c|) + eps (6 + C_SIN |s| + C_COS |c|) + the argument-reduction term of sin and cos ],
             dk = 2 e_P / |rel| + 3 eps the direction error of the axis (e_P / n_xy for theta's axis), s, c of the angle
  A_n        (e_V_n + e_V_{n-1}) / h + (3/2) eps (|V_n| + |V_{n-1}|) / h
  unit_rel, tension, angle_proj: first order from e_P, e_V through the quotients, + 2 eps of the value's terms
  midpoint   the mean of the two nodes' uncertainties + eps/2 of the mean of the two magnitudes
  delay slot exact nodes: the scaling alone.

A step is undecided -- not compared -- when (a) its scale exceeds 1e-3 of its own increment |theta* - theta_n| (u kappa > 1e-3
with kappa = 1 / |theta* - theta_n| the step's condition number: the bound then says nothing about the increment), (b) a
discontinuous branch (n_xy < 1e-9, n_th < 1e-9) has its exact argument within its own budget of the threshold, (c) a slope
leaves T's finite range or an operation's domain, or an input is not finite (NaN nodes are compared as NaN by the tests).

Margin.  M_STEP is twice the largest ratio, over table(), of the float64 oracle's own one-step error to this scale
(orc.rollout_vec's node n + 1 against step_true on the oracle's own nodes), never below 4; with eps32 for fp32, as
cable_reference.py does.  tests/test_rollout_reference_host.py measures it again and fails if the oracle leaves M_STEP / 2."""
import ast
import collections
import functools
import math

import mpmath as mp
import numpy as np
from mpmath import mpf

import cable_reference as cr
import expr_reference as er

DPS = 50
M_STEP = 4.0                    # measured: largest ratio of the float64 oracle 0.232 (theta), 0.206 (gamma); 2 x 0.232 < 4
UND_KAPPA = 1e-3
AXIS_EPS = 1e-9
TRIG_FAST_LIMIT = 2.0 ** 26     # device_math.h (fp64): a sine argument beyond this leaves the two-term reduction
K_TABLE = 19                    # one full 16-wide workgroup and a ragged one
B_RK4 = (1, 2, 2, 1)

StepRef = collections.namedtuple("StepRef", "th ga scale_th scale_ga und_th und_ga")


# ---- slopes ------------------------------------------------------------------------------------------------------------------
class SlotEvaluator(er.Evaluator):
    """expr_reference.Evaluator on slots that are mpf values with an uncertainty each (a plain Evaluator takes slots that T
    holds exactly)."""

    def __call__(self, vals, errs):
        self.vals, self.errs = vals, errs
        try:
            with mp.workdps(DPS + 10):
                return self._ev(self.tree)
        except er._Undefined:
            return None, None

    def _ev(self, node):
        if isinstance(node, ast.Name):
            i = int(node.id[1:])
            v = self.vals[i]
            if v is None or not mp.isfinite(v):
                raise er._Undefined
            return v, float(self.errs[i])
        return super()._ev(node)


@functools.lru_cache(maxsize=None)
def _evaluator(text, fmt):
    return SlotEvaluator(text, er.FMT[fmt])


def _text(f):
    return f if isinstance(f, str) else f.expr


# ---- small vector helpers (mpf) ------------------------------------------------------------------------------------------------
def _trig_err(F, x, s, c):
    """Own error of the device sine and cosine of an exact x (DESIGN section 3's table, the unit of expr_reference)."""
    Ps, hs = er._half_ulp_lo(F, False)
    Pc, hc = er._half_ulp_lo(F, True)
    ax = float(abs(x))
    return (er.C_SIN[F.name] * (F.eps * float(abs(s)) + ax / Ps * hs), er.C_COS[F.name] * (F.eps * float(abs(c)) + ax / Pc * hc))


def _rot(F, v, ev, axis, dk, ang):
    """Rodrigues rotation of v (2-norm uncertainty ev) about a unit axis with direction error dk by the exact angle ang."""
    s, c = mp.sin(ang), mp.cos(ang)
    es, ec = _trig_err(F, ang, s, c)
    out = cr._rod(v, axis, ang)
    nv = float(cr._norm(v))
    e = ev + nv * (dk * (float(abs(s)) + 2 * float(abs(1 - c))) + 6 * F.eps + es + ec)
    return out, e


class Rollout:
    """One candidate's step references: the inputs rounded to T once, V and the feature rows cached per node."""

    def __init__(self, cfg, model, state, U_k, nodes, fmt="f64", Rtab=None):
        self.F = F = er.FMT[fmt]
        self.cfg = cfg
        r = self.r = lambda x: mpf(float(F.np(x)))
        with mp.workdps(DPS):
            st = np.asarray(state.as_array() if hasattr(state, "as_array") else state, dtype=np.float64)
            self.P0 = [r(x) for x in st[0:3]]
            self.P1 = [r(x) for x in st[3:6]]
            self.V1 = [r(x) for x in st[6:9]]
            self.A1 = [r(x) for x in st[9:12]]
            self.prev = (r(st[14]), r(st[15]))
            self.h, self.vs = r(cfg.dt), r(cfg.v_scale)
            self.mean = [r(x) for x in model.mean]
            self.scale = [r(x) for x in model.scale]
            self.U = [[r(x) for x in row] for row in np.asarray(U_k, dtype=np.float64)]
            self.finite = bool(np.all(np.isfinite(np.asarray(U_k, dtype=np.float64))) and np.all(np.isfinite(st)))
            self.nodes = np.asarray(nodes, dtype=np.float64)
            self.Rtab = None if Rtab is None else [[[r(x) for x in row] for row in R] for R in np.asarray(Rtab, dtype=np.float64)]
            self.c8, self.lo, self.hi = r(1e-8), r(1e-5), r(10.0)
        self.ft, self.fg = _evaluator(_text(model.f_theta), fmt), _evaluator(_text(model.f_gamma), fmt)
        self._P, self._V, self._X = {}, {}, {}
        self.branch_close = set()               # nodes whose axes sit within their budget of a threshold

    def node(self, m):
        """(theta, gamma) of node m as mpf; node -1 is the state's delay pair."""
        if m < 0:
            return self.prev
        return mpf(float(self.nodes[m, 0])), mpf(float(self.nodes[m, 1]))

    # -- kinematics ------------------------------------------------------------------------------------------------------------
    def P(self, m):
        """(P_m exact, per-component uncertainty)."""
        if m not in self._P:
            eps = self.F.eps
            k = self.vs * self.h
            val = [self.P1[i] + k * sum((self.U[j][i] for j in range(m)), mpf(0)) for i in range(3)]
            mag = [float(abs(self.P1[i]) + abs(k) * sum((abs(self.U[j][i]) for j in range(m)), mpf(0))) for i in range(3)]
            self._P[m] = (val, [0.0 if m == 0 else 0.5 * (m + 3) * eps * a for a in mag])
        return self._P[m]

    def _axes(self, m):
        """theta and gamma axes of node m with their direction errors; notes a threshold within the budget."""
        eps = self.F.eps
        P, eP = self.P(m)
        rel = [P[i] - self.P0[i] for i in range(3)]
        e_rel = [eP[i] + 0.5 * eps * float(abs(rel[i])) for i in range(3)]
        nxy = mp.sqrt(rel[0] ** 2 + rel[1] ** 2)
        nr = cr._norm(rel)
        e_xy = e_rel[0] + e_rel[1] + 2 * eps * float(nxy)
        thr = mpf(AXIS_EPS)
        if abs(nxy - thr) <= e_xy:
            self.branch_close.add(m)
        if nxy < thr:
            xy, dk_t = [mpf(1), mpf(0), mpf(0)], 0.0
        else:
            xy, dk_t = [rel[0] / nxy, rel[1] / nxy, mpf(0)], 2 * (e_rel[0] + e_rel[1]) / float(nxy) + 3 * eps
        th = cr._cross(xy, [mpf(0), mpf(0), mpf(1)])
        nth = cr._norm(th)
        if abs(nth - thr) <= 4 * eps + dk_t:
            self.branch_close.add(m)
        th = [mpf(0), mpf(1), mpf(0)] if nth < thr else [x / nth for x in th]
        if nr == 0:
            return th, None, dk_t, 0.0
        return th, [x / nr for x in rel], dk_t, 2 * sum(e_rel) / float(nr) + 3 * eps

    def V(self, m):
        """(V_m exact given the nodes, 2-norm uncertainty): the state's V1 at node 0, the transform of U_{m-1} after it."""
        if m not in self._V:
            F, eps = self.F, self.F.eps
            if m == 0:
                self._V[m] = (self.V1, 0.0)
            else:
                Uw = self.U[m - 1]
                if self.cfg.vt_mode == 0:
                    self._V[m] = (list(Uw), 0.0)
                elif self.cfg.vt_mode == 2:
                    R = self.Rtab[m - 1]
                    val = [sum((R[i][j] * Uw[j] for j in range(3)), mpf(0)) for i in range(3)]
                    e = [2.5 * eps * float(sum((abs(R[i][j] * Uw[j]) for j in range(3)), mpf(0))) for i in range(3)]
                    self._V[m] = (val, math.sqrt(sum(x * x for x in e)))
                else:
                    th, ga = self.node(m - 1)
                    tha, gaa, dk_t, dk_g = self._axes(m - 1)
                    if gaa is None:
                        self._V[m] = (None, 0.0)                  # rel = 0: the gamma axis is 0 / 0
                    else:
                        v, e = _rot(F, list(Uw), 0.0, gaa, dk_g, -ga)
                        v, e = _rot(F, v, e, tha, dk_t, th)
                        self._V[m] = (v, e)
        return self._V[m]

    # -- feature rows ------------------------------------------------------------------------------------------------------------
    def exo(self, m):
        """(values, uncertainties) of the 14 exogenous slots of node m, or None where a value is undefined."""
        if m in self._X:
            return self._X[m]
        eps, cfg = self.F.eps, self.cfg
        P, eP = self.P(m)
        V, eV = self.V(m)
        if V is None:
            self._X[m] = None
            return None
        if m == 0:
            A, eA = self.A1, [0.0] * 3
        else:
            W, eW = self.V(m - 1)
            if W is None:
                self._X[m] = None
                return None
            A = [(V[i] - W[i]) / self.h for i in range(3)]
            eA = [float((eV + eW + 1.5 * eps * (abs(V[i]) + abs(W[i]))) / self.h) for i in range(3)]
        eVc = [eV] * 3
        rel = [P[i] - self.P0[i] for i in range(3)]
        e_rel = [eP[i] + 0.5 * eps * float(abs(rel[i])) for i in range(3)]
        nr = cr._norm(rel)
        e_nr = (sum(float(abs(rel[i])) * e_rel[i] for i in range(3)) / float(nr) if nr > 0 else sum(e_rel)) + 2 * eps * float(nr)
        d = nr + self.c8
        unit = [rel[i] / d for i in range(3)]
        e_unit = [float(e_rel[i] / d + abs(unit[i]) / d * (e_nr + 0.5 * eps * float(d))) + eps * float(abs(unit[i])) for i in range(3)]
        tension = min(max(nr, self.lo), self.hi)
        nv = cr._norm(V)
        dv = nv + self.c8
        num = sum((V[i] * unit[i] for i in range(3)), mpf(0))
        mag = float(sum((abs(V[i] * unit[i]) for i in range(3)), mpf(0)))
        e_num = sum(float(abs(V[i])) * e_unit[i] + float(abs(unit[i])) * eVc[i] for i in range(3)) + 2 * eps * mag
        ap = num / dv
        e_ap = float(e_num / dv + abs(ap) / dv * (eV + 2 * eps * float(nv) + 0.5 * eps * float(dv))) + eps * float(abs(ap))
        raw = P + V + A + unit
        e_raw = eP + eVc + eA + e_unit
        if cfg.feature_map == 1:
            vals = [(raw[i] - self.mean[i]) / self.scale[i] for i in range(12)]
            errs = [self._scaled(raw[i], e_raw[i], i) for i in range(12)]
            vals += [mpf(0), (ap - self.mean[16]) / self.scale[16]]
            errs += [0.0, self._scaled(ap, e_ap, 16)]
        else:
            raw = raw + [tension, min(max(ap, mpf(-1)), mpf(1))]
            e_raw = e_raw + [e_nr, e_ap]
            vals = [(raw[i] - self.mean[i]) / self.scale[i] for i in range(14)]
            errs = [self._scaled(raw[i], e_raw[i], i) for i in range(14)]
        self._X[m] = (vals, errs)
        return self._X[m]

    def _scaled(self, raw, e_raw, i):
        return float((e_raw + 2 * self.F.eps * (abs(raw) + abs(self.mean[i]))) / abs(self.scale[i]))

    # -- the step ----------------------------------------------------------------------------------------------------------------
    def step(self, n):
        """StepRef of the step from node n to node n + 1."""
        with mp.workdps(DPS):
            return self._step(n)

    def _step(self, n):
        F, eps, cfg, h = self.F, self.F.eps, self.cfg, self.h
        bad = StepRef(None, None, None, None, True, True)
        if not self.finite or not np.all(np.isfinite(self.nodes[max(n - 2, 0):n + 1])):
            return bad
        xa, xb = self.exo(n), self.exo(n + 1)
        if xa is None or xb is None:
            return bad
        th, ga = self.node(n)
        thm, gam = self.node(n - 1)
        gen2 = cfg.feature_map == 1
        mean, scale = self.mean, self.scale
        xm = ([(a + b) / 2 for a, b in zip(*(xa[0], xb[0]))],
              [(a + b) / 2 + 0.25 * eps * float(abs(u) + abs(v)) for a, b, u, v in zip(xa[1], xb[1], xa[0], xb[0])])

        def delay(c):
            if gen2:
                return [], []
            sa = [(thm - mean[16]) / scale[16], (gam - mean[17]) / scale[17]]
            sb = [(th - mean[16]) / scale[16], (ga - mean[17]) / scale[17]]
            ea = [self._scaled(thm, 0.0, 16), self._scaled(gam, 0.0, 17)]
            eb = [self._scaled(th, 0.0, 16), self._scaled(ga, 0.0, 17)]
            if cfg.prev_mode == 1 or c == 0:
                return sa, ea
            if c == 2:
                return sb, eb
            return ([(a + b) / 2 for a, b in zip(sa, sb)],
                    [(u + v) / 2 + 0.25 * eps * float(abs(a) + abs(b)) for u, v, a, b in zip(ea, eb, sa, sb)])

        def stage(yth, yga, e_th, e_ga, c):
            exo = (xa, xm, xb)[c]
            if gen2:
                cy, sg = mp.cos(yth), mp.sin(yga)
                _, ecos = _trig_err(F, yth, mp.sin(yth), cy)
                esin, _ = _trig_err(F, yga, sg, mp.cos(yga))
                vals = list(exo[0][:12]) + [(yth - mean[12]) / scale[12], (yga - mean[13]) / scale[13], (cy - mean[14]) / scale[14],
                                            (sg - mean[15]) / scale[15], exo[0][13]]
                errs = list(exo[1][:12]) + [self._scaled(yth, e_th, 12), self._scaled(yga, e_ga, 13),
                                            self._scaled(cy, e_th * float(abs(mp.sin(yth))) + ecos, 14),
                                            self._scaled(sg, e_ga * float(abs(mp.cos(yga))) + esin, 15), exo[1][13]]
            else:
                dv, de = delay(c)
                vals = list(exo[0]) + [(yth - mean[14]) / scale[14], (yga - mean[15]) / scale[15]] + dv
                errs = list(exo[1]) + [self._scaled(yth, e_th, 14), self._scaled(yga, e_ga, 15)] + de
            kt, Bt = self.ft(vals, errs)
            kg, Bg = self.fg(vals, errs)
            if kt is None or kg is None:
                return None
            return kt, kg, Bt, Bg

        k = [stage(th, ga, 0.0, 0.0, 0)]
        if k[0] is None:
            return bad
        if cfg.integrator == 1:
            b, c = (1,), h
        else:
            b, c = B_RK4, h / 6
            for a, cc in ((mpf(1) / 2, 1), (mpf(1) / 2, 1), (mpf(1), 2)):
                kt, kg, Bt, Bg = k[-1]
                yth, yga = th + a * h * kt, ga + a * h * kg
                e_th = eps * float(abs(yth)) + float(a * h) * (eps * float(abs(kt)) + Bt)
                e_ga = eps * float(abs(yga)) + float(a * h) * (eps * float(abs(kg)) + Bg)
                k.append(stage(yth, yga, e_th, e_ga, cc))
                if k[-1] is None:
                    return bad
        th_n = th + c * sum((bj * kj[0] for bj, kj in zip(b, k)), mpf(0))
        ga_n = ga + c * sum((bj * kj[1] for bj, kj in zip(b, k)), mpf(0))
        cf = float(c)
        s_th = eps * float(abs(th) + abs(th_n)) + cf * sum(bj * (eps * float(abs(kj[0])) + kj[2]) for bj, kj in zip(b, k))
        s_ga = eps * float(abs(ga) + abs(ga_n)) + cf * sum(bj * (eps * float(abs(kj[1])) + kj[3]) for bj, kj in zip(b, k))
        close = cfg.vt_mode == 1 and any(m in self.branch_close for m in (n - 2, n - 1, n))
        und_th = close or not s_th <= UND_KAPPA * float(abs(th_n - th))
        und_ga = close or not s_ga <= UND_KAPPA * float(abs(ga_n - ga))
        return StepRef(th_n, ga_n, s_th, s_ga, und_th, und_ga)


def step_true(cfg, model, state, U_k, nodes, n, Rtab=None, fmt="f64"):
    """(theta*, gamma*) of node n + 1 as mpf (None, None where the step is undefined): see the module text."""
    s = Rollout(cfg, model, state, U_k, nodes, fmt, Rtab).step(n)
    return s.th, s.ga


def step_ratios(cfg, model, state, U, traj, fmt="f64", Rtab=None, n_max=None, limit=None):
    """Per candidate and step: |node n + 1 - reference| / scale for theta and gamma (NaN where undecided), and |theta* -
    theta_n|.  `limit`: steps are compared while |theta_n| and |gamma_n| stay below it."""
    U = np.asarray(U, dtype=np.float64)
    traj = np.asarray(traj, dtype=np.float64)
    K, N = U.shape[0], U.shape[1]
    N = N if n_max is None else min(N, n_max)
    rt = np.full((K, N), np.nan); rg = np.full((K, N), np.nan); dth = np.full((K, N), np.nan)
    with mp.workdps(DPS):
        for k in range(K):
            ro = Rollout(cfg, model, state, U[k], traj[k], fmt, Rtab)
            for n in range(N):
                if limit is not None and not (abs(traj[k, n, 0]) < limit and abs(traj[k, n, 1]) < limit):
                    break
                s = ro.step(n)
                if s.th is None:
                    continue
                dth[k, n] = float(abs(s.th - mpf(float(traj[k, n, 0]))))
                got_t, got_g = float(traj[k, n + 1, 0]), float(traj[k, n + 1, 1])
                if not s.und_th:
                    rt[k, n] = float(abs(mpf(got_t) - s.th)) / s.scale_th if math.isfinite(got_t) else np.inf
                if not s.und_ga:
                    rg[k, n] = float(abs(mpf(got_g) - s.ga)) / s.scale_ga if math.isfinite(got_g) else np.inf
    return rt, rg, dth


def worst(rt, rg):
    """Largest decided ratio of a (theta, gamma) pair of ratio tables (0 where nothing is decided)."""
    both = np.concatenate([np.ravel(rt), np.ravel(rg)])
    both = both[~np.isnan(both)]
    return float(both.max()) if both.size else 0.0


# ---- cost terms on a returned trajectory ---------------------------------------------------------------------------------------
def cost_term_true(cfg, which, U_k, nodes, fmt="f64"):
    """J* of one candidate with the single weight `which` ("w_theta", "w_gamma", "w_u") non-zero, at 50 digits, from the
    returned nodes (from U for w_u).  Bound: (N + 3) eps J* -- N additions of non-negative terms, a subtraction, a square and
    the weight per term."""
    F = er.FMT[fmt]
    r = lambda x: mpf(float(F.np(x)))
    with mp.workdps(DPS):
        w = r(getattr(cfg, which))
        J = mpf(0)
        N = len(U_k)
        for n in range(N):
            if which == "w_theta":
                J += w * (mpf(float(nodes[n + 1][0])) - r(cfg.theta_ref)) ** 2
            elif which == "w_gamma":
                J += w * (mpf(float(nodes[n + 1][1])) - r(cfg.gamma_ref)) ** 2
            else:
                J += w * sum(((r(U_k[n][i]) - r(cfg.U_ref[i])) ** 2 for i in range(3)), mpf(0))
        return J, (N + 3) * F.eps * float(J)


def full_cost_true(cfg, state, U_k, nodes, fmt="f64"):
    """The default-weight J of one candidate on the returned nodes, with its bound: the three quadratic terms as above, the
    tension and the lowest point from cable_reference with their own bounds (M_T, M_Z and their conditioning scales)."""
    F = er.FMT[fmt]
    eps = F.eps
    r = lambda x: mpf(float(F.np(x)))
    with mp.workdps(DPS):
        st = np.asarray(state, dtype=np.float64)
        P0 = [r(x) for x in st[0:3]]
        P = [r(x) for x in st[3:6]]
        k = r(cfg.v_scale) * r(cfg.dt)
        J, bound = mpf(0), 0.0
        L, up = float(F.np(cfg.L)), float(cfg.up)
        for n in range(len(U_k)):
            P = [P[i] + k * r(U_k[n][i]) for i in range(3)]
            th, ga = float(nodes[n + 1][0]), float(nodes[n + 1][1])
            rel = [P[i] - P0[i] for i in range(3)]
            l = mp.sqrt(rel[0] ** 2 + rel[1] ** 2); dH = mpf(up) * rel[2]; d = cr._norm(rel)
            quad = r(cfg.w_theta) * (mpf(th) - r(cfg.theta_ref)) ** 2 + r(cfg.w_gamma) * (mpf(ga) - r(cfg.gamma_ref)) ** 2 \
                + r(cfg.w_u) * sum(((r(U_k[n][i]) - r(cfg.U_ref[i])) ** 2 for i in range(3)), mpf(0))
            root = cr._root_mp(l, dH, mpf(L))
            w = mpf(float(F.np(cfg.cable_wet_weight))) / mpf(L)
            if root is not None and cfg.c_lo <= root[1] <= cfg.c_hi:
                T = w * l / (2 * mp.sinh(root[0]))
                kap = float(cr._kappa_mp(root[0], root[2], dH, mpf(L)))
                eT = cr.M_T * eps * (1 + kap * float(root[0] / mp.tanh(root[0]))) * float(T)
            else:
                T = w * l / 2
                eT = cr.M_T * eps * float(T)
            z = cr.lowest_z_true([float(x) for x in P0], [float(x) for x in P], th, ga, L, cfg.n_shape_pts, up, cfg.c_lo, cfg.c_hi)
            eZ = cr.M_Z * cr.z_scale(z.kappa, L, eps)
            taut = max(mpf(0), d - r(cfg.rho_taut) * mpf(L))
            flo = max(mpf(0), mpf(up) * (r(cfg.z_floor) - z.z))
            J += quad + r(cfg.w_T) * T + r(cfg.w_taut) * taut ** 2 + r(cfg.w_floor) * flo ** 2
            bound += 4 * eps * float(quad) + float(cfg.w_T) * eT + float(cfg.w_taut) * 2 * float(taut) * 4 * eps * float(d + L) \
                + float(cfg.w_floor) * 2 * float(flo) * eZ
        return J, bound + (len(U_k) + 3) * eps * float(J)


# ---- the deterministic workspace -----------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "tag state U")

OPERATING = ((-0.0342, -0.0522), (0.0, -0.0), (0.6, -0.6), (-0.6, 0.05), (1.5, 0.3), (-3.0, 1.0), (math.pi / 2, -math.pi / 2), (12.5, -7.0))


def _scaler():
    import json
    import os
    s = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaler.json")))
    return np.array(s["mean"]), np.array(s["scale"])


def controls(N, K=K_TABLE, seed=0):
    """Scaler-statistics draws with rows scaled x20 and x40, an all-zero row, a constant row and a duplicate pair mixed in."""
    mean, scale = _scaler()
    rng = np.random.default_rng(7300 + seed)
    U = mean[3:6] + scale[3:6] * rng.standard_normal((K, N, 3))
    if K >= 6:
        U[1 % K] *= 20.0
        U[2 % K] *= 40.0
        U[3 % K] = 0.0
        U[4 % K] = U[4 % K][0]
        U[K - 1] = U[0]                       # a duplicate pair in two workgroups (K > 16)
    if K >= 19:
        U[17] *= 20.0                       # big steps in the ragged workgroup too
    return U


def _state(op, prev, rel, V, P0=(0.0, 0.0, 0.0)):
    th, ga = OPERATING[op]
    P0 = np.asarray(P0, float)
    return np.concatenate([P0, P0 + np.asarray(rel, float), np.asarray(V, float), np.zeros(3), [th, ga, th - prev, ga + prev]])


@functools.lru_cache(maxsize=None)
def table(N=20):
    """The workspace: 18 state rows that cover every operating point, connection vector and velocity of the list, each with the
    mixed control set; the huge-sine set (one control of 3e10) and the set with a NaN candidate."""
    mean, _ = _scaler()
    rm, Vm = mean[0:3], mean[3:6]
    unit = rm / np.linalg.norm(rm)
    rel = {"mean": rm, "+x": (1.2, 0.0, 0.0), "vertical": (0.0, 0.0, -1.4), "nxy=1e-3": (1e-3 * 0.6, -1e-3 * 0.8, -1.1),
           "|rel|=1e-9": 1e-9 * unit, "|rel|=1e-6": 1e-6 * unit, "|rel|=12": 12.0 * unit}
    vel = {"mean": Vm, "zero": np.zeros(3), "par": 50.0 * unit, "anti": -50.0 * unit, "x1e3": 1e3 * Vm}
    P0 = (0.4, -0.3, 0.25)
    spec = [(0, 0.0, "mean", "mean", None), (1, 0.0, "+x", "zero", None), (2, 0.01, "mean", "mean", None),
            (3, 0.05, "vertical", "par", None), (4, 0.0, "mean", "mean", None), (5, 0.1, "nxy=1e-3", "anti", None),
            (6, 0.0, "mean", "mean", P0), (7, 0.3, "mean", "x1e3", None), (2, 0.0, "|rel|=1e-9", "mean", None),
            (4, 0.02, "|rel|=1e-6", "zero", None), (3, 0.0, "|rel|=12", "mean", None), (2, 0.03, "+x", "par", P0),
            (4, 0.0, "vertical", "anti", None), (0, 0.0, "nxy=1e-3", "x1e3", None), (1, 0.2, "|rel|=12", "par", None),
            (6, 0.05, "+x", "mean", None), (5, 0.0, "mean", "zero", None), (7, 0.0, "|rel|=1e-6", "mean", None)]
    rows = []
    for i, (op, prev, r, v, p0) in enumerate(spec):
        tag = "%d:(%g,%g)%+g rel=%s V=%s%s" % (i, OPERATING[op][0], OPERATING[op][1], prev, r, v, " P0" if p0 else "")
        rows.append(Row(tag, _state(op, prev, rel[r], vel[v], p0 or (0.0, 0.0, 0.0)), controls(N, seed=i)))
    U = controls(N, seed=100)
    U[HUGE_CANDIDATE, min(2, N - 1), 0] = 3e10
    rows.append(Row("huge:(0.6,-0.6) one control of 3e10", _state(2, 0.0, rm, Vm), U))
    U = controls(N, seed=101)
    U[NAN_CANDIDATE] = np.nan
    rows.append(Row("nan:(1.5,0.3) candidate 6 NaN", _state(4, 0.0, rm, Vm), U))
    return tuple(rows)


HUGE_ROW, NAN_ROW, NAN_CANDIDATE, HUGE_CANDIDATE = 18, 19, 6, 5
