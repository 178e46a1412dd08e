"""``MPC``: the shooting controller the reference's call surface implies (``step(state) -> u``).

The reference ships no solver (its ``pympc`` submodule is empty); this class supplies one
whose per-step work is the fused HIP rollout kernel: sample / take K candidate control
sequences, roll all of them over the horizon, return the first control of the cheapest.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .engine import Engine, MPCConfig, MPCState, StepResult, state_array
from .model import DynamicsModel, default_model


class GaussianSampler:
    """U[k, n, :] = mean + std * N(0, 1), i.i.d.; candidate 0 may be pinned to a warm start."""

    def __init__(self, mean=None, std=None, seed: int = 20250523):
        m = default_model()
        self.mean = np.asarray(mean if mean is not None else m.mean[3:6], float)      # scaler x3..x5
        self.std = np.asarray(std if std is not None else m.scale[3:6], float)
        self.rng = np.random.default_rng(seed)

    def sample(self, K: int, N: int, dtype=np.float64, warm_start: Optional[np.ndarray] = None) -> np.ndarray:
        U = (self.mean + self.std * self.rng.standard_normal((K, N, 3))).astype(dtype, copy=False)
        if warm_start is not None:
            U[0] = warm_start
        return U


class DeviceGaussianSampler:
    """The same candidate law drawn on the GPU by the library itself (``rovmpc_mpc_step_sampled``): standard normals from
    Philox4x32-10 keyed by (seed, step counter) through Box-Muller, so a step is a pure function of (state, seed, step) and
    reproducible on the host (the test oracle restates the law).  The candidate tensor never exists on the host."""

    def __init__(self, mean=None, std=None, seed: int = 20250523):
        m = default_model()
        self.mean = np.ascontiguousarray(mean if mean is not None else m.mean[3:6], dtype=np.float64)
        self.std = np.ascontiguousarray(std if std is not None else m.scale[3:6], dtype=np.float64)
        self.seed = int(seed)
        self.step = 0


class MPC:
    """``mpc = MPC(N=20, K=4096); u = mpc.step(state)``.

    ``state``: :class:`MPCState`, a dict of its fields, or 16 floats
    (P0, P1, V1, A1, theta, gamma, theta_prev, gamma_prev).
    After ``step`` the full result (u, predicted (theta, gamma) trajectory, cost, index) is in
    ``mpc.last``.  Pass ``U`` (K, N, 3) to evaluate given candidates instead of sampling.
    """

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None,
                 sampler: Optional[GaussianSampler] = None, warm_start: bool = True, device_sampling: bool = False,
                 **overrides):
        self.engine = Engine(cfg, model, **overrides)
        self.cfg = self.engine.cfg
        self.sampler = sampler or GaussianSampler()
        self.warm_start = warm_start
        self.last: Optional[StepResult] = None
        self._best_seq: Optional[np.ndarray] = None
        self._dev = None
        if device_sampling:
            # candidates are drawn, rolled out and reduced on the GPU by one library call; the host sees the state and the record
            self._dev = sampler if isinstance(sampler, DeviceGaussianSampler) else DeviceGaussianSampler()

    def _step_device_sampled(self, state) -> np.ndarray:
        d = self._dev
        rec = self.engine.mpc_step_sampled(state, d.seed, d.step, d.mean, d.std, self.warm_start)
        d.step += 1
        self.last = StepResult.from_record(rec, self.cfg.N)
        return self.last.u

    def step(self, state, U: Optional[np.ndarray] = None) -> np.ndarray:
        if U is None and self._dev is not None:
            return self._step_device_sampled(state)
        if U is None:
            ws = None
            if self.warm_start and self._best_seq is not None:
                ws = np.vstack([self._best_seq[1:], self._best_seq[-1:]])          # shifted previous optimum
            U = self.sampler.sample(self.cfg.K, self.cfg.N, self.cfg.np_dtype, ws)
        res = self.engine.step(state, U)
        self.last = res
        self._best_seq = np.asarray(U[res.index], dtype=np.float64).copy()
        return res.u

    def rollout_costs(self, state, U, return_traj: bool = False):
        return self.engine.rollout_costs(state, U, return_traj)

    def close(self):
        self.engine.close()


@dataclass
class PlanLoopResult:
    """The rows of a device-resident loop (``run``), split.  Single controller: records (T, result_len), plans (T, N, 3),
    stats (T, 4), and for CEM spreads (T, N, 3) and elites (T, n_elite) int64 (None for MPPI); batched: a problem axis after T.
    ``plans`` are nu* (MPPI) or mu* (CEM), ``stats`` as ``rovmpc_mppi_step`` / ``rovmpc_cem_step`` return them."""
    records: np.ndarray
    plans: np.ndarray
    stats: np.ndarray
    spreads: Optional[np.ndarray] = None
    elites: Optional[np.ndarray] = None

    @property
    def u(self) -> np.ndarray:
        return self.records[..., 2:5]

    @property
    def cost(self) -> np.ndarray:
        return self.records[..., 0]


def loop_feedback(feedback) -> bool:
    """feedback of a ``run``: a bool, or 0 / 1."""
    if not isinstance(feedback, (bool, np.bool_)) and not (isinstance(feedback, (int, np.integer)) and feedback in (0, 1)):
        raise ValueError(f"feedback must be False / True (or 0 / 1), got {feedback!r}")
    return bool(feedback)


def loop_rows(rows) -> np.ndarray:
    """(T, 16) float64, T >= 1: the measured rows of a single controller's ``run`` (``closed_loop_inputs``)."""
    r = np.ascontiguousarray(rows, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != 16 or r.shape[0] < 1:
        raise ValueError(f"rows must have shape (T, 16) with T >= 1, got {r.shape}")
    return r


def loop_rows_batch(rows, B: int) -> np.ndarray:
    """(B, T, 16) float64 from (B, T, 16), or from (T, 16) given to every problem."""
    r = np.asarray(rows, dtype=np.float64)
    if r.ndim == 2:
        r = np.broadcast_to(loop_rows(r), (B,) + r.shape)
    if r.ndim != 3 or r.shape[0] != B or r.shape[2] != 16 or r.shape[1] < 1:
        raise ValueError(f"rows must have shape ({B}, T, 16) or (T, 16) with T >= 1, got {r.shape}")
    return np.array(r, dtype=np.float64, order="C")


def split_rows(rows: np.ndarray, R: int, N: int, n_elite: Optional[int] = None) -> PlanLoopResult:
    """Rows (..., W) of a loop into their parts: W = R + 3N + 4 (MPPI), or R + 6N + 4 + n_elite (CEM, the elites int64)."""
    lead, C3 = rows.shape[:-1], 3 * N
    rec, plans = rows[..., :R].copy(), rows[..., R:R + C3].reshape(lead + (N, 3)).copy()
    if n_elite is None:
        assert rows.shape[-1] == R + C3 + 4
        return PlanLoopResult(rec, plans, rows[..., R + C3:].copy())
    assert rows.shape[-1] == R + 2 * C3 + 4 + n_elite
    return PlanLoopResult(rec, plans, rows[..., R + 2 * C3:R + 2 * C3 + 4].copy(),
                          rows[..., R + C3:R + 2 * C3].reshape(lead + (N, 3)).copy(),
                          np.ascontiguousarray(rows[..., R + 2 * C3 + 4:]).view(np.int64).copy())


def _run_on_device(engine, rows: np.ndarray, W: int, lead: tuple, call) -> np.ndarray:
    """Upload the measured rows, run ``call(d_exo, d_rows)``, download the loop's rows (lead + (W,))."""
    import torch
    dev = torch.device("cuda", engine.cfg.device)
    exo = torch.tensor(rows, device=dev)
    out = torch.empty(lead + (W,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    call(exo.data_ptr(), out.data_ptr())
    return out.cpu().numpy()


def _stats_dict(names, stats: np.ndarray) -> dict:
    """``last_stats`` from stats (4,) of a single controller (scalars) or (B, 4) of a batched one (columns); n_finite counts."""
    if stats.ndim == 1:
        return {k: int(v) if k == "n_finite" else float(v) for k, v in zip(names, stats)}
    return {k: stats[:, i].astype(np.int64) if k == "n_finite" else stats[:, i].copy() for i, k in enumerate(names)}


def _default_std(std) -> np.ndarray:
    return np.asarray(std if std is not None else default_model().scale[3:6], dtype=np.float64)


def _config_value(cfg, overrides: dict, name: str) -> int:
    """N or K of the engine a controller is about to make, for the checks that come before it exists."""
    return int(overrides[name]) if name in overrides else getattr(cfg if cfg is not None else MPCConfig(), name)


class NavCost:
    """``NavCost(track, w_pos=..., w_term=..., w_du=..., w_sphere=..., spheres=..., origin=0)``: the navigation cost of the
    plan controllers (include/rovmpc.h, rovmpc_set_nav_cost).  ``track`` (Tr, 3), or (B, Tr, 3) for a batched controller: row
    j is where the vehicle's P1 should be, in metres, at control step ``origin + j`` (the controller's ``step_count``); before
    the origin the first row holds, past the end the last one, and a single row is a waypoint.  Each candidate's predicted
    path P_{n+1} = P_n + v_scale dt U_n adds to its cost: ``w_pos`` times the squared distance to the track on every node,
    ``w_term`` on the last node, ``w_du`` times the squared control increments along the horizon and ``w_sphere`` times the
    squared penetration into each of up to 8 ``spheres`` (cx, cy, cz, R).  A scalar weight is repeated on the three channels.
    The values are checked here (ValueError), before any library call."""

    def __init__(self, track, w_pos=0.0, w_term=0.0, w_du=0.0, w_sphere=0.0, spheres=(), origin=0):
        self.c_nav, self.tracks = _lib.nav_cost(track, w_pos, w_term, w_du, w_sphere, spheres, origin)
        self.w_pos, self.w_term, self.w_du = (np.array(v) for v in (self.c_nav.w_pos, self.c_nav.w_term, self.c_nav.w_du))
        self.w_sphere, self.origin = float(self.c_nav.w_sphere), int(self.c_nav.origin)
        self.spheres = np.array(self.c_nav.spheres).reshape(-1, 4)[:self.c_nav.n_spheres].copy()


def check_nav(nav, B: int, batched: bool):
    """nav of a controller with B problems, before the library is called: None or a NavCost with 1 or (batched) B tracks."""
    if nav is None:
        return None
    if not isinstance(nav, NavCost):
        raise TypeError("nav must be a rovmpc.NavCost or None")
    Bt = nav.tracks.shape[0]
    if Bt != 1 and not (batched and Bt == B):
        raise ValueError(f"the track must be (Tr, 3){f' or ({B}, Tr, 3)' if batched else ''}, got {nav.tracks.shape}")
    return nav


class TetherCost:
    """``TetherCost(spheres, w, margin=0.0)``: the tether keep-out cost of the plan controllers (include/rovmpc.h,
    rovmpc_set_tether_cost).  ``spheres`` (n, 4), 1 <= n <= 8: (cx, cy, cz, R) in metres.  At every predicted node the
    cable's shape -- the augmented catenary from the anchor P0 to the vehicle's predicted position under the node's
    predicted (theta, gamma), ``n_shape_pts`` samples joined by segments -- adds ``w`` times its squared penetration into
    each sphere grown by ``margin``.  The values are checked here (ValueError / TypeError), before any library call."""

    def __init__(self, spheres, w, margin=0.0):
        self.c_tether = _lib.tether_cost(spheres, w, margin)
        self.w, self.margin = float(self.c_tether.w), float(self.c_tether.margin)
        self.spheres = np.array(self.c_tether.spheres).reshape(-1, 4)[:self.c_tether.n_spheres].copy()


def check_tether(tether):
    """tether of a controller, before the library is called: None or a TetherCost."""
    if tether is not None and not isinstance(tether, TetherCost):
        raise TypeError("tether must be a rovmpc.TetherCost or None")
    return tether


class _PlanController:
    """What the four controllers share: an engine of their own, the seed and step counter of the draws, the plan's shape
    and the result of the last step.  The single-problem form; _BatchedPlanController overrides what a batch changes."""

    _batch = ""         # "_batch": the engine's batched entries

    def __init__(self, cfg, model, seed: int, overrides: dict, beta=None, lo=None, hi=None, nav=None, tether=None):
        self.seed = int(seed)
        self.tether = check_tether(tether)
        self.beta, self.box = _lib.noise_correlation(beta), _lib.control_box(lo, hi)      # ValueError before the library is called
        self.nav = check_nav(nav, getattr(self, "B", 1), bool(self._batch))
        self.engine = Engine(cfg, model, **overrides)
        self.cfg = self.engine.cfg
        if self.beta is not None:
            self.engine.set_noise_correlation(self.beta)
        if self.box is not None:
            self.engine.mppi_set_bounds(*self.box)
        if self.nav is not None:
            self.engine.set_nav_cost(self.nav.c_nav, self.nav.tracks)
        if self.tether is not None:
            self.engine.set_tether_cost(self.tether.c_tether)
        self._default_mean = np.asarray(default_model().mean[3:6], dtype=np.float64)
        self.step_count = 0
        self.last = self.last_stats = None       # StepResult (batched: a list of them), dict

    def set_nav(self, nav):
        """Set (a ``NavCost``) or clear (None) the navigation cost; it holds from the next ``step`` or ``run``, whose
        ``step_count`` is the control step the track is read at."""
        nav = check_nav(nav, getattr(self, "B", 1), bool(self._batch))
        if nav is None:
            self.engine.set_nav_cost(None)
        else:
            self.engine.set_nav_cost(nav.c_nav, nav.tracks)
        self.nav = nav

    def set_tether(self, tether):
        """Set (a ``TetherCost``) or clear (None) the tether keep-out cost; it holds from the next ``step`` or ``run``."""
        tether = check_tether(tether)
        self.engine.set_tether_cost(None if tether is None else tether.c_tether)
        self.tether = tether

    def _entry(self, name: str):
        """engine.mppi_step, engine.cem_reset_batch, ..."""
        return getattr(self.engine, f"{self._kind}_{name}{self._batch}")

    def _plan(self, value, name: str) -> np.ndarray:
        """(N, 3) from (N, 3), from (3,) repeated on every node, or from None (the scaler mean of x3..x5)."""
        N = self.cfg.N
        plan = self._default_mean if value is None else np.asarray(value, dtype=np.float64)
        if plan.shape == (3,):
            plan = np.tile(plan, (N, 1))
        if plan.shape != (N, 3):
            raise ValueError(f"{name} must have shape ({N}, 3) or (3,), got {plan.shape}")
        return plan

    def _seeds(self):
        return self.seed

    def _states(self, state):
        return state

    def _loop_rows(self, rows) -> np.ndarray:
        return loop_rows(rows)

    def _took_step(self, rec, stats: dict) -> np.ndarray:
        self.step_count += 1
        self.last = StepResult.from_record(rec, self.cfg.N)
        self.last_stats = stats
        return self.last.u

    def _run(self, rows, feedback) -> PlanLoopResult:
        """The loop of ``run``; leaves everything but the plan as T calls of ``step`` would."""
        r, fb = self._loop_rows(rows), loop_feedback(feedback)
        e, T = self.engine, r.shape[-2]
        loop = getattr(e, f"{self._kind}_closed_loop{self._batch}_device")
        out = _run_on_device(e, r, self._row_len(), (T,) + r.shape[:-2], lambda d_exo, d_rows: loop(
            d_exo, T, fb, self._seeds(), self.step_count, self.params, d_rows))
        res = self._split(out)
        self._took_step(res.records[-1].copy(), _stats_dict(self._stats, res.stats[-1]))
        self.step_count += T - 1
        return res

    def close(self):
        self.engine.close()


class _MPPILaw:
    """What MPPI and BatchedMPPI share: the parameters, the engine's mppi_* entries and the layout of a loop's row."""

    _kind, _stats = "mppi", ("rho", "eta", "ess", "J0")

    def _row_len(self) -> int:
        return self.engine.mppi_row_len()

    def _split(self, rows) -> PlanLoopResult:
        return split_rows(rows, self.engine.result_len, self.cfg.N)

    def _set_params(self, lam, std, n_iter):
        self.std = _default_std(std)
        self.params = _lib.MPPIParams.make(n_iter, lam, self.std)        # ValueError before the library is called
        self.lam, self.n_iter = float(lam), int(n_iter)
        self.nominal: Optional[np.ndarray] = None

    def reset(self, nominal=None):
        """Set the nominal plan ((N, 3), or (3,) repeated on every node; batched: (B, N, 3) too; default: the scaler mean)."""
        nu = self._plan(nominal, "nominal")
        self._entry("reset")(nu)
        self.nominal = nu.copy()

    def step(self, state) -> np.ndarray:
        rec, self.nominal, stats = self._entry("step")(self._states(state), self._seeds(), self.step_count, self.params)
        return self._took_step(rec, _stats_dict(self._stats, stats))

    def run(self, rows, feedback: bool = False) -> PlanLoopResult:
        """T = len(rows) control steps by one library call, the plant update on the GPU (rovmpc_mppi_closed_loop_device):
        ``rows`` (T, 16) measured states; ``feedback``: from the second step on (theta, gamma) are the model's own first
        predicted node.  Row i is what ``step`` would return on the state the plant rule gives; ``step`` and ``run``
        interleave (the step counter advances by T).  Batched (rovmpc_mppi_closed_loop_batch_device): ``rows`` (B, T, 16), or
        (T, 16) given to every problem; the arrays are (T, B, ...), problem b's those of ``MPPI(seed=seeds[b],
        nominal=nominal[b]).run(rows[b])``."""
        res = self._run(rows, feedback)
        self.nominal = res.plans[-1].copy()
        return res


class _CEMLaw:
    """What CEM and BatchedCEM share: the parameters, the engine's cem_* entries and the layout of a loop's row."""

    _kind, _stats = "cem", ("J_best", "J_worst_elite", "n_finite", "J0")

    def _row_len(self) -> int:
        return self.engine.cem_row_len(self.n_elite)

    def _split(self, rows) -> PlanLoopResult:
        return split_rows(rows, self.engine.result_len, self.cfg.N, self.n_elite)

    def _set_params(self, cfg, overrides, n_elite, n_iter, alpha, std, std_min, lo, hi, reserved):
        K = _config_value(cfg, overrides, "K")
        if n_elite is None:
            n_elite = max(K // 64, 1)
        if isinstance(n_elite, bool) or int(n_elite) != n_elite or int(n_elite) > K:
            raise ValueError(f"n_elite must be an integer <= K = {K} (got {n_elite!r})")
        self.params = _lib.CEMParams.make(n_iter, n_elite, alpha, _default_std(std), std_min, lo, hi, reserved)   # ValueError before the library is called
        self.n_iter, self.n_elite, self.alpha = int(n_iter), int(n_elite), float(alpha)
        self.mean = self.std = self.elites = None

    def reset(self, mean=None):
        """Set the mean plan ((N, 3), or (3,) repeated on every node; batched: (B, N, 3) too; default: the scaler mean)."""
        mu = self._plan(mean, "mean")
        self._entry("reset")(mu)
        self.mean = mu.copy()

    def step(self, state) -> np.ndarray:
        rec, self.mean, self.std, self.elites, stats = self._entry("step")(self._states(state), self._seeds(), self.step_count, self.params)
        return self._took_step(rec, _stats_dict(self._stats, stats))

    def run(self, rows, feedback: bool = False) -> PlanLoopResult:
        """T control steps by one library call (rovmpc_cem_closed_loop_device / _batch_device); see ``MPPI.run``."""
        res = self._run(rows, feedback)
        self.mean, self.std, self.elites = res.plans[-1].copy(), res.spreads[-1].copy(), res.elites[-1].copy()
        return res


class MPPI(_MPPILaw, _PlanController):
    """``mppi = MPPI(N=20, K=4096, lam=1.0); u = mppi.step(state)``: model-predictive path integral control.

    The handle keeps a nominal plan (N, 3); each step samples K candidates around it on the GPU (candidate 0 = the nominal),
    rolls them out, moves the nominal to the exp(-J/lam)-weighted mean of all candidates (``n_iter`` times, without a
    host round trip) and returns its first control.  The law is stated in include/rovmpc.h (rovmpc_mppi_step).
    Defaults: nominal = the scaler mean of x3..x5 on every node, std = its scale.  After ``step``: ``last`` (the record of
    the last rollout, with u = nominal*[0]), ``last_stats`` (rho, eta, ess, J0), ``nominal`` (the plan the step returned).
    ``beta`` (3 values in [0, 1), default None: white noise) makes the sampling noise AR(1) along the horizon, unit variance
    and corr(n, m) = beta^|n - m| per channel: smoother candidates.  ``lo``, ``hi`` (default None: unbounded) box the controls:
    candidates, nominal and the returned control lie inside exactly (rovmpc_set_noise_correlation, rovmpc_mppi_set_bounds).
    ``nav`` (a ``NavCost``, default None) adds path-tracking, rate and keep-out costs of the vehicle's predicted path; the
    track is read at ``step_count``, which ``step`` advances by 1 and ``run`` by T (``set_nav`` changes or clears it).
    ``tether`` (a ``TetherCost``, default None) keeps the predicted cable shapes out of spheres (``set_tether``).
    """

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, lam: float = 1.0, std=None,
                 n_iter: int = 1, seed: int = 20250523, nominal=None, beta=None, lo=None, hi=None, nav=None, tether=None,
                 **overrides):
        self._set_params(lam, std, n_iter)
        super().__init__(cfg, model, seed, overrides, beta, lo, hi, nav, tether)
        self.reset(nominal)


class CEM(_CEMLaw, _PlanController):
    """``cem = CEM(N=20, K=4096, n_elite=64); u = cem.step(state)``: the cross-entropy method.

    The handle keeps a mean plan (N, 3); each step samples K candidates on the GPU around it with a per-node spread, clamped
    to the box [lo, hi] (candidate 0 = the clamped mean), rolls them out, keeps the ``n_elite`` cheapest (by rank only, ties to
    the lower index) and refits mean and spread from them (``n_iter`` times, without a host round trip); it returns the
    clamped first control of the mean.  The law is stated in include/rovmpc.h (rovmpc_cem_step).
    Defaults: mean = the scaler mean of x3..x5 on every node, std = its scale, std_min = 0, bounds +-inf, alpha = 0,
    n_elite = K / 64 (at least 1).  After ``step``: ``last`` (the record of the last rollout, with u = clamp(mean*[0])),
    ``last_stats`` (J_best, J_worst_elite, n_finite, J0), ``mean`` and ``std`` (the plan and spread the step returned) and
    ``elites`` (the last iteration's elite indices in rank order, -1 padded).  ``beta`` as for ``MPPI``: AR(1) sampling noise;
    ``nav`` and ``tether`` as for ``MPPI``: the navigation and the tether keep-out cost.
    """

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, n_elite: Optional[int] = None,
                 n_iter: int = 1, alpha: float = 0.0, std=None, std_min=(0.0, 0.0, 0.0), lo=(-np.inf,) * 3, hi=(np.inf,) * 3,
                 seed: int = 20250523, mean=None, reserved: int = 0, beta=None, nav=None, tether=None, **overrides):
        self._set_params(cfg, overrides, n_elite, n_iter, alpha, std, std_min, lo, hi, reserved)
        super().__init__(cfg, model, seed, overrides, beta, nav=nav, tether=tether)
        self.reset(mean)


BATCH_MAX = 1024      # problems of a batched controller (PLAN_BATCH_MAX of the library)


def batch_plans(value, B: int, N: int, default, name: str) -> np.ndarray:
    """(B, N, 3) from (B, N, 3), from (N, 3) or (3,) repeated, or from None (``default`` (3,) on every node)."""
    plan = np.asarray(default if value is None else value, dtype=np.float64)
    if plan.shape not in ((3,), (N, 3), (B, N, 3)):
        raise ValueError(f"{name} must have shape ({B}, {N}, 3), ({N}, 3) or (3,), got {plan.shape}")
    return np.array(np.broadcast_to(plan, (B, N, 3)), dtype=np.float64, order="C")      # a copy of its own


def batch_seeds(seeds, seed: int, B: int) -> np.ndarray:
    """(B,) uint64: the given seeds, or seed + b."""
    if seeds is None:
        return (np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.arange(B, dtype=np.uint64)).astype(np.uint64)
    if len(seeds) != B:
        raise ValueError(f"seeds must have length B = {B} (got {len(seeds)})")
    return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds], dtype=np.uint64)


def batch_states(states, B: int) -> np.ndarray:
    """(B, 16) from an array of that shape or from a sequence of B MPCState / dicts / 16 floats."""
    if isinstance(states, np.ndarray) and states.ndim == 2:
        st = np.ascontiguousarray(states, dtype=np.float64)
    else:
        st = np.stack([state_array(v) for v in states]) if len(states) else np.empty((0, 16))
    if st.shape != (B, 16):
        raise ValueError(f"states must be (B, 16) = ({B}, 16) or a sequence of {B} states, got {st.shape}")
    return st


def check_batch(B, seed: int, seeds, plan, N: int, name: str):
    """B, the seeds and the shape of the plans of a batched controller, checked before an engine exists (ValueError);
    returns (B, seeds (B,) uint64)."""
    if isinstance(B, bool) or int(B) != B or not 1 <= int(B) <= BATCH_MAX:
        raise ValueError(f"B must be an integer in 1..{BATCH_MAX} (got {B!r})")
    B = int(B)
    sd = batch_seeds(seeds, seed, B)
    if plan is not None and np.shape(plan) not in ((3,), (N, 3), (B, N, 3)):
        raise ValueError(f"{name} must have shape ({B}, {N}, 3), ({N}, 3) or (3,), got {np.shape(plan)}")
    return B, sd


class _BatchedPlanController(_PlanController):
    """What BatchedMPPI and BatchedCEM share on top of _PlanController: B, the seeds and the per-problem results."""

    _batch = "_batch"

    def __init__(self, cfg, model, B, seed: int, seeds, plan, name: str, overrides: dict, beta=None, lo=None, hi=None, nav=None,
                 tether=None):
        self.B, self.seeds = check_batch(B, seed, seeds, plan, _config_value(cfg, overrides, "N"), name)
        super().__init__(cfg, model, int(self.seeds[0]), overrides, beta, lo, hi, nav, tether)
        self.records: Optional[np.ndarray] = None

    def _seeds(self):
        return self.seeds

    def _plan(self, value, name: str) -> np.ndarray:
        return batch_plans(value, self.B, self.cfg.N, self._default_mean, name)

    def _states(self, states) -> np.ndarray:
        return batch_states(states, self.B)

    def _loop_rows(self, rows) -> np.ndarray:
        return loop_rows_batch(rows, self.B)

    def _took_step(self, records, stats: dict) -> np.ndarray:
        self.step_count += 1
        self.records = records
        self.last = [StepResult.from_record(r, self.cfg.N) for r in records]
        self.last_stats = stats
        return records[:, 2:5].copy()

    def candidates(self):
        """Host copies of the last iteration's candidates U (B, K, N, 3) and costs J (B, K)."""
        return self._entry("last")()


class BatchedMPPI(_MPPILaw, _BatchedPlanController):
    """``ctl = BatchedMPPI(B=64, N=20, K=4096, lam=1.0); u = ctl.step(states)``: B independent MPPI plans, each with its own
    state, seed (default ``seed + b``) and warm-started nominal, advanced by one library call per control step; lam, std and
    n_iter are shared.  Problem b's results are bit for bit those of ``MPPI(seed=seeds[b], nominal=nominal[b])`` on its own
    (include/rovmpc.h, rovmpc_mppi_step_batch).  ``nominal``: (B, N, 3), or (N, 3) / (3,) repeated; default the scaler mean.
    ``step(states)`` takes (B, 16) or a sequence of B states and returns u (B, 3).  After it: ``records`` (B, result_len),
    ``last`` (a list of StepResult), ``nominal`` (B, N, 3), ``last_stats`` (rho, eta, ess, J0: arrays of length B).
    ``beta``, ``lo``, ``hi`` as for ``MPPI``, shared by the batch; ``nav`` too, its track (Tr, 3) shared or (B, Tr, 3) per problem; ``tether`` shared by the batch."""

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, B: int, lam: float = 1.0,
                 std=None, n_iter: int = 1, seed: int = 20250523, seeds=None, nominal=None, beta=None, lo=None, hi=None, nav=None,
                 tether=None, **overrides):
        self._set_params(lam, std, n_iter)
        super().__init__(cfg, model, B, seed, seeds, nominal, "nominal", overrides, beta, lo, hi, nav, tether)
        self.reset(nominal)


class BatchedCEM(_CEMLaw, _BatchedPlanController):
    """``ctl = BatchedCEM(B=64, N=20, K=4096, n_elite=64); u = ctl.step(states)``: B independent CEM plans, each with its own
    state, seed (default ``seed + b``) and warm-started mean, advanced by one library call per control step; the parameters
    of ``CEM`` are shared.  Problem b's results are bit for bit those of ``CEM(seed=seeds[b], mean=mean[b])`` on its own
    (include/rovmpc.h, rovmpc_cem_step_batch).  After ``step``: ``records``, ``last`` (a list of StepResult), ``mean`` and
    ``std`` (B, N, 3), ``elites`` (B, n_elite), ``last_stats`` (J_best, J_worst_elite, n_finite, J0: arrays of length B).
    ``beta``, ``nav`` and ``tether`` as for ``BatchedMPPI``."""

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, B: int,
                 n_elite: Optional[int] = None, n_iter: int = 1, alpha: float = 0.0, std=None, std_min=(0.0, 0.0, 0.0),
                 lo=(-np.inf,) * 3, hi=(np.inf,) * 3, seed: int = 20250523, seeds=None, mean=None, reserved: int = 0, beta=None,
                 nav=None, tether=None, **overrides):
        self._set_params(cfg, overrides, n_elite, n_iter, alpha, std, std_min, lo, hi, reserved)
        super().__init__(cfg, model, B, seed, seeds, mean, "mean", overrides, beta, nav=nav, tether=tether)
        self.reset(mean)


def synthetic_problem(K: int, N: int, seed: int = 20250523, dtype=np.float64):
    """The synthetic MPC step of SURVEY section 8(d) / BASELINE.md section 3: state at the scaler means,
    candidates drawn from the scaler statistics of x3..x5.  Returns (state(16,), U(K,N,3))."""
    m = default_model()
    rng = np.random.default_rng(seed)
    P1 = m.mean[0:3] + 0.05 * rng.standard_normal(3)
    st = MPCState(P0=(0.0, 0.0, 0.0), P1=P1, V1=m.mean[3:6], A1=(0.0, 0.0, 0.0),
                  theta=-0.0342, gamma=-0.0522, theta_prev=-0.0342, gamma_prev=-0.0522)
    U = m.mean[3:6] + m.scale[3:6] * rng.standard_normal((K, N, 3))
    return st.as_array(), U.astype(dtype, copy=False)
