"""``MPC``: the shooting controller the reference's call surface implies (``step(state) -> u``).

The reference ships no solver (its ``pympc`` submodule is empty); this class supplies one
whose per-step work is the fused HIP rollout kernel: sample / take K candidate control
sequences, roll all of them over the horizon, return the first control of the cheapest.
"""
from __future__ import annotations

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


class _PlanController:
    """What MPPI and CEM share: an engine of their own, the seed and step counter of the draws, the plan's shape and the
    result of the last step."""

    def __init__(self, cfg, model, seed: int, overrides: dict):
        self.seed = int(seed)
        self.engine = Engine(cfg, model, **overrides)
        self.cfg = self.engine.cfg
        self._default_mean = np.asarray(default_model().mean[3:6], dtype=np.float64)
        self.step_count = 0
        self.last: Optional[StepResult] = None
        self.last_stats: Optional[dict] = None

    def _plan(self, value, name: str) -> np.ndarray:
        """(N, 3) from (N, 3), from (3,) repeated on every node, or from None (the scaler mean of x3..x5)."""
        N = self.cfg.N
        plan = self._default_mean if value is None else np.asarray(value, dtype=np.float64)
        if plan.shape == (3,):
            plan = np.tile(plan, (N, 1))
        if plan.shape != (N, 3):
            raise ValueError(f"{name} must have shape ({N}, 3) or (3,), got {plan.shape}")
        return plan

    def _took_step(self, rec, stats: dict) -> np.ndarray:
        self.step_count += 1
        self.last = StepResult.from_record(rec, self.cfg.N)
        self.last_stats = stats
        return self.last.u

    def close(self):
        self.engine.close()


class MPPI(_PlanController):
    """``mppi = MPPI(N=20, K=4096, lam=1.0); u = mppi.step(state)``: model-predictive path integral control.

    The handle keeps a nominal plan (N, 3); each step samples K candidates around it on the GPU (candidate 0 = the nominal),
    rolls them out, moves the nominal to the exp(-J/lam)-weighted mean of all candidates (``n_iter`` times, without a
    host round trip) and returns its first control.  The law is stated in include/rovmpc.h (rovmpc_mppi_step).
    Defaults: nominal = the scaler mean of x3..x5 on every node, std = its scale.  After ``step``: ``last`` (the record of
    the last rollout, with u = nominal*[0]), ``last_stats`` (rho, eta, ess, J0), ``nominal`` (the plan the step returned).
    """

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, lam: float = 1.0, std=None,
                 n_iter: int = 1, seed: int = 20250523, nominal=None, **overrides):
        self.std = np.asarray(std if std is not None else default_model().scale[3:6], dtype=np.float64)
        self.params = _lib.MPPIParams.make(n_iter, lam, self.std)        # ValueError before the library is called
        self.lam, self.n_iter = float(lam), int(n_iter)
        super().__init__(cfg, model, seed, overrides)
        self.nominal: Optional[np.ndarray] = None
        self.reset(nominal)

    def reset(self, nominal=None):
        """Set the nominal plan ((N, 3), or (3,) repeated on every node; default: the scaler mean of x3..x5)."""
        nu = self._plan(nominal, "nominal")
        self.engine.mppi_reset(nu)
        self.nominal = nu.copy()

    def step(self, state) -> np.ndarray:
        rec, self.nominal, stats = self.engine.mppi_step(state, self.seed, self.step_count, self.params)
        return self._took_step(rec, {"rho": float(stats[0]), "eta": float(stats[1]), "ess": float(stats[2]), "J0": float(stats[3])})


class CEM(_PlanController):
    """``cem = CEM(N=20, K=4096, n_elite=64); u = cem.step(state)``: the cross-entropy method.

    The handle keeps a mean plan (N, 3); each step samples K candidates on the GPU around it with a per-node spread, clamped
    to the box [lo, hi] (candidate 0 = the clamped mean), rolls them out, keeps the ``n_elite`` cheapest (by rank only, ties to
    the lower index) and refits mean and spread from them (``n_iter`` times, without a host round trip); it returns the
    clamped first control of the mean.  The law is stated in include/rovmpc.h (rovmpc_cem_step).
    Defaults: mean = the scaler mean of x3..x5 on every node, std = its scale, std_min = 0, bounds +-inf, alpha = 0,
    n_elite = K / 64 (at least 1).  After ``step``: ``last`` (the record of the last rollout, with u = clamp(mean*[0])),
    ``last_stats`` (J_best, J_worst_elite, n_finite, J0), ``mean`` and ``std`` (the plan and spread the step returned) and
    ``elites`` (the last iteration's elite indices in rank order, -1 padded).
    """

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, n_elite: Optional[int] = None,
                 n_iter: int = 1, alpha: float = 0.0, std=None, std_min=(0.0, 0.0, 0.0), lo=(-np.inf,) * 3, hi=(np.inf,) * 3,
                 seed: int = 20250523, mean=None, reserved: int = 0, **overrides):
        K = int(overrides["K"]) if "K" in overrides else (cfg.K if cfg is not None else MPCConfig().K)
        if n_elite is None:
            n_elite = max(K // 64, 1)
        if isinstance(n_elite, bool) or int(n_elite) != n_elite or int(n_elite) > K:
            raise ValueError(f"n_elite must be an integer <= K = {K} (got {n_elite!r})")
        std = np.asarray(std if std is not None else default_model().scale[3:6], dtype=np.float64)
        self.params = _lib.CEMParams.make(n_iter, n_elite, alpha, std, std_min, lo, hi, reserved)   # ValueError before the library is called
        self.n_iter, self.n_elite, self.alpha = int(n_iter), int(n_elite), float(alpha)
        super().__init__(cfg, model, seed, overrides)
        self.mean: Optional[np.ndarray] = None
        self.std: Optional[np.ndarray] = None
        self.elites: Optional[np.ndarray] = None
        self.reset(mean)

    def reset(self, mean=None):
        """Set the mean plan ((N, 3), or (3,) repeated on every node; default: the scaler mean of x3..x5)."""
        mu = self._plan(mean, "mean")
        self.engine.cem_reset(mu)
        self.mean = mu.copy()

    def step(self, state) -> np.ndarray:
        rec, self.mean, self.std, self.elites, stats = self.engine.cem_step(state, self.seed, self.step_count, self.params)
        return self._took_step(rec, {"J_best": float(stats[0]), "J_worst_elite": float(stats[1]), "n_finite": int(stats[2]),
                                     "J0": float(stats[3])})


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


def _config_N(cfg, overrides) -> int:
    return int(overrides["N"]) if "N" in overrides else (cfg.N if cfg is not None else MPCConfig().N)


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

    def __init__(self, cfg, model, B, seed: int, seeds, plan, name: str, overrides: dict):
        self.B, self.seeds = check_batch(B, seed, seeds, plan, _config_N(cfg, overrides), name)
        super().__init__(cfg, model, int(self.seeds[0]), overrides)
        self.records: Optional[np.ndarray] = None

    def _plans(self, value, name: str) -> np.ndarray:
        return batch_plans(value, self.B, self.cfg.N, self._default_mean, name)

    def _took_steps(self, records, stats: dict) -> np.ndarray:
        self.step_count += 1
        self.records = records
        self.last = [StepResult.from_record(r, self.cfg.N) for r in records]
        self.last_stats = stats
        return records[:, 2:5].copy()


class BatchedMPPI(_BatchedPlanController):
    """``ctl = BatchedMPPI(B=64, N=20, K=4096, lam=1.0); u = ctl.step(states)``: B independent MPPI plans, each with its own
    state, seed (default ``seed + b``) and warm-started nominal, advanced by one library call per control step; lam, std and
    n_iter are shared.  Problem b's results are bit for bit those of ``MPPI(seed=seeds[b], nominal=nominal[b])`` on its own
    (include/rovmpc.h, rovmpc_mppi_step_batch).  ``nominal``: (B, N, 3), or (N, 3) / (3,) repeated; default the scaler mean.
    ``step(states)`` takes (B, 16) or a sequence of B states and returns u (B, 3).  After it: ``records`` (B, result_len),
    ``last`` (a list of StepResult), ``nominal`` (B, N, 3), ``last_stats`` (rho, eta, ess, J0: arrays of length B)."""

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, B: int, lam: float = 1.0,
                 std=None, n_iter: int = 1, seed: int = 20250523, seeds=None, nominal=None, **overrides):
        self.std = np.asarray(std if std is not None else default_model().scale[3:6], dtype=np.float64)
        self.params = _lib.MPPIParams.make(n_iter, lam, self.std)        # ValueError before the library is called
        self.lam, self.n_iter = float(lam), int(n_iter)
        super().__init__(cfg, model, B, seed, seeds, nominal, "nominal", overrides)
        self.nominal: Optional[np.ndarray] = None
        self.reset(nominal)

    def reset(self, nominal=None):
        nu = self._plans(nominal, "nominal")
        self.engine.mppi_reset_batch(nu)
        self.nominal = nu.copy()

    def step(self, states) -> np.ndarray:
        st = batch_states(states, self.B)
        rec, self.nominal, stats = self.engine.mppi_step_batch(st, self.seeds, self.step_count, self.params)
        return self._took_steps(rec, {"rho": stats[:, 0].copy(), "eta": stats[:, 1].copy(), "ess": stats[:, 2].copy(),
                                      "J0": stats[:, 3].copy()})

    def candidates(self):
        """Host copies of the last iteration's candidates U (B, K, N, 3) and costs J (B, K)."""
        return self.engine.mppi_last_batch()


class BatchedCEM(_BatchedPlanController):
    """``ctl = BatchedCEM(B=64, N=20, K=4096, n_elite=64); u = ctl.step(states)``: B independent CEM plans, each with its own
    state, seed (default ``seed + b``) and warm-started mean, advanced by one library call per control step; the parameters
    of ``CEM`` are shared.  Problem b's results are bit for bit those of ``CEM(seed=seeds[b], mean=mean[b])`` on its own
    (include/rovmpc.h, rovmpc_cem_step_batch).  After ``step``: ``records``, ``last`` (a list of StepResult), ``mean`` and
    ``std`` (B, N, 3), ``elites`` (B, n_elite), ``last_stats`` (J_best, J_worst_elite, n_finite, J0: arrays of length B)."""

    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, *, B: int,
                 n_elite: Optional[int] = None, n_iter: int = 1, alpha: float = 0.0, std=None, std_min=(0.0, 0.0, 0.0),
                 lo=(-np.inf,) * 3, hi=(np.inf,) * 3, seed: int = 20250523, seeds=None, mean=None, reserved: int = 0, **overrides):
        K = int(overrides["K"]) if "K" in overrides else (cfg.K if cfg is not None else MPCConfig().K)
        if n_elite is None:
            n_elite = max(K // 64, 1)
        if isinstance(n_elite, bool) or int(n_elite) != n_elite or int(n_elite) > K:
            raise ValueError(f"n_elite must be an integer <= K = {K} (got {n_elite!r})")
        std = np.asarray(std if std is not None else default_model().scale[3:6], dtype=np.float64)
        self.params = _lib.CEMParams.make(n_iter, n_elite, alpha, std, std_min, lo, hi, reserved)   # ValueError before the library is called
        self.n_iter, self.n_elite, self.alpha = int(n_iter), int(n_elite), float(alpha)
        super().__init__(cfg, model, B, seed, seeds, mean, "mean", overrides)
        self.mean: Optional[np.ndarray] = None
        self.std: Optional[np.ndarray] = None
        self.elites: Optional[np.ndarray] = None
        self.reset(mean)

    def reset(self, mean=None):
        mu = self._plans(mean, "mean")
        self.engine.cem_reset_batch(mu)
        self.mean = mu.copy()

    def step(self, states) -> np.ndarray:
        st = batch_states(states, self.B)
        rec, self.mean, self.std, self.elites, stats = self.engine.cem_step_batch(st, self.seeds, self.step_count, self.params)
        return self._took_steps(rec, {"J_best": stats[:, 0].copy(), "J_worst_elite": stats[:, 1].copy(),
                                      "n_finite": stats[:, 2].astype(np.int64), "J0": stats[:, 3].copy()})

    def candidates(self):
        """Host copies of the last iteration's candidates U (B, K, N, 3) and costs J (B, K)."""
        return self.engine.cem_last_batch()


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
