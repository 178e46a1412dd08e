"""``Engine``: one librovmpc handle (one GPU, one stream, one workspace) with NumPy / device
pointer entry points.  Everything numeric happens in the HIP library."""
from __future__ import annotations

import collections
import ctypes as C
import enum
from dataclasses import dataclass, field, asdict, replace
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Config, State, MPPIParams, CEMParams, FitParams, TrackParams, RovmpcError, check, load_library
from .model import DynamicsModel, default_model


@dataclass
class MPCConfig:
    """Mirror of ``rovmpc_config`` (include/rovmpc.h).  Defaults = SURVEY section 8(d) synthetic
    set-up, except dt (1/60 s: the learned gamma equation is a finite difference at the
    data rate) and non-zero w_T / w_floor so every cost term is live."""
    N: int = 20
    K: int = 4096
    dtype: str = "f64"
    device: int = 0
    n_shape_pts: int = 16
    vt_mode: int = _lib.VT_COMPOSE
    prev_mode: int = _lib.PREV_INTERP
    integrator: int = _lib.RK4
    frame: str = "ENU"
    force_interpreter: bool = False
    candidates_per_block: int = 0
    threads_per_block: int = 0
    debug_flags: int = 0
    jit: bool = True             # specialise non-default models with hiprtc at set_model
    no_builtin: bool = False     # never substitute the compiled-in kernel for the reference's chosen rows
    feature_map: int = _lib.FEATURES_GEN1   # FEATURES_GEN2: 17 unscaled slots of simulate_rk4_theta_gamma.py:12-42
    dt: float = 1.0 / 60.0
    v_scale: float = 1e-3
    L: float = 3.0
    cable_wet_weight: float = 1.521
    c_lo: float = 1e-6
    c_hi: float = 10.0
    w_theta: float = 1.0
    w_gamma: float = 1.0
    w_u: float = 1e-6
    w_T: float = 1e-2
    w_taut: float = 1e3
    rho_taut: float = 0.98
    w_floor: float = 10.0
    z_floor: float = -1.2
    theta_ref: float = 0.0
    gamma_ref: float = 0.0
    U_ref: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    def to_c(self) -> Config:
        if self.dtype not in ("f64", "f32"):
            raise ValueError("dtype must be 'f64' or 'f32'")
        if self.frame not in ("ENU", "NED"):
            raise ValueError("frame must be 'ENU' or 'NED'")
        c = Config()
        c.struct_size = C.sizeof(Config)
        c.device = self.device
        c.dtype = _lib.F64 if self.dtype == "f64" else _lib.F32
        c.N, c.K, c.n_shape_pts = self.N, self.K, self.n_shape_pts
        c.vt_mode, c.prev_mode, c.integrator = self.vt_mode, self.prev_mode, self.integrator
        c.frame = _lib.ENU if self.frame == "ENU" else _lib.NED
        c.force_interpreter = int(self.force_interpreter)
        c.candidates_per_block = self.candidates_per_block
        c.threads_per_block = self.threads_per_block
        c.debug_flags = self.debug_flags
        c.jit_off = 0 if self.jit else 1
        c.no_builtin = int(self.no_builtin)
        c.feature_map = self.feature_map
        for k in ("dt", "v_scale", "L", "cable_wet_weight", "c_lo", "c_hi", "w_theta", "w_gamma", "w_u", "w_T",
                  "w_taut", "rho_taut", "w_floor", "z_floor", "theta_ref", "gamma_ref"):
            setattr(c, k, float(getattr(self, k)))
        c.U_ref = (C.c_double * 3)(*[float(v) for v in self.U_ref])
        return c

    @property
    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32


@dataclass
class MPCState:
    """Feature-slot values at horizon node 0 (``rovmpc_state``): P0 rod_end [m], P1 ROV cable
    attach point [m], V1 rob_cor_speed, A1 its time derivative, theta, gamma and their
    previous samples (simply.py:15-41)."""
    P0: Sequence[float] = (0.0, 0.0, 0.0)
    P1: Sequence[float] = (0.0, 0.0, 0.0)
    V1: Sequence[float] = (0.0, 0.0, 0.0)
    A1: Sequence[float] = (0.0, 0.0, 0.0)
    theta: float = 0.0
    gamma: float = 0.0
    theta_prev: Optional[float] = None
    gamma_prev: Optional[float] = None

    def as_array(self) -> np.ndarray:
        tp = self.theta if self.theta_prev is None else self.theta_prev
        gp = self.gamma if self.gamma_prev is None else self.gamma_prev
        a = np.concatenate([np.asarray(self.P0, float), np.asarray(self.P1, float), np.asarray(self.V1, float),
                            np.asarray(self.A1, float), [self.theta, self.gamma, tp, gp]])
        if a.shape != (16,):
            raise ValueError("P0, P1, V1, A1 must have 3 components each")
        return a

    def with_markers(self, markers, guess=None, engine: Optional["Engine"] = None) -> "MPCState":
        """A copy whose theta and gamma are fitted to the cable markers (M, 3) of this state's P0 and P1
        (``Engine.fit_theta_gamma``; ``guess`` (theta, gamma): the start, by default this state's own angles).  Raises
        ValueError naming the status unless the fit is CONVERGED.  ``engine``: the one whose L, bracket and frame hold
        (default: the shared helper engine)."""
        if guess is None:
            guess = (self.theta, self.gamma)
        fit = (engine or default_engine()).fit_theta_gamma(self.P0, self.P1, markers, guess=guess)
        status = FitStatus(int(fit.status))
        if status is not FitStatus.CONVERGED:
            raise ValueError(f"marker fit did not converge: status {status.name} after {int(fit.iters)} trial steps (rms {float(fit.rms):g} m)")
        return replace(self, theta=float(fit.theta), gamma=float(fit.gamma))


class FitStatus(enum.IntEnum):
    """``rovmpc_fit_status`` (include/rovmpc.h)."""
    CONVERGED = 0
    MAX_ITER = 1
    DEGENERATE = 2
    CHORD = 3
    TOO_FEW = 4
    NONFINITE = 5


CableFit = collections.namedtuple("CableFit", "theta gamma rms rms0 iters status")
CableFit.__doc__ = """Columns of ``rovmpc_fit_theta_gamma``'s out: arrays (B,), or scalars for one frame; iters and status integers."""


class TrackState(enum.IntEnum):
    """``rovmpc_track_state`` (include/rovmpc.h)."""
    LOCKED = 0
    ACQUIRED = 1
    HELD = 2
    NONE = 3


@dataclass(frozen=True)
class CableTrack:
    """Columns of ``rovmpc_track_markers``'s out, arrays (T,) for one recording or (B, T): theta, gamma, theta_prev,
    gamma_prev, rms (NaN where no attempt was accepted), iters (trial steps summed over the frame's attempts), status
    (``FitStatus`` of the accepted or else the last attempt), state (``TrackState``), start (index into the start list, -1 =
    the carry); and ``carry`` (2,) or (B, 2): the last accepted estimate, NaN if none, to hand to the next call."""
    theta: np.ndarray
    gamma: np.ndarray
    theta_prev: np.ndarray
    gamma_prev: np.ndarray
    rms: np.ndarray
    iters: np.ndarray
    status: np.ndarray
    state: np.ndarray
    start: np.ndarray
    carry: np.ndarray

    def rows(self, rows, allow_missing: bool = False) -> np.ndarray:
        """A copy of the state rows (T, 16) or (B, T, 16) -- what ``MPPI.run`` and the closed loops consume -- with slots
        12..15 (theta, gamma, theta_prev, gamma_prev) filled from the track.  A frame whose state is NONE has no angles:
        ValueError, unless ``allow_missing``, which leaves those rows as given."""
        out = np.array(rows, dtype=np.float64)
        if out.shape != self.theta.shape + (16,):
            raise ValueError(f"rows must be {self.theta.shape + (16,)}, got {out.shape}")
        ok = self.state != TrackState.NONE
        if not allow_missing and not ok.all():
            raise ValueError(f"{int((~ok).sum())} frame(s) have no estimate (track state NONE), the first at index "
                             f"{tuple(int(i) for i in np.argwhere(~ok)[0])}")
        for slot, col in zip(range(12, 16), (self.theta, self.gamma, self.theta_prev, self.gamma_prev)):
            out[..., slot] = np.where(ok, col, out[..., slot])
        return out


def state_array(state) -> np.ndarray:
    if isinstance(state, MPCState):
        return state.as_array()
    if isinstance(state, dict):
        return MPCState(**state).as_array()
    a = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
    if a.shape != (16,):
        raise ValueError("state must be an MPCState, a dict of its fields or 16 floats")
    return a


def _c_state(a: np.ndarray) -> State:
    s = State()
    C.memmove(C.byref(s), a.ctypes.data, 16 * 8)
    return s


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclass
class StepResult:
    u: np.ndarray          # (3,)  first control of the best candidate
    traj: np.ndarray       # (N+1, 2) predicted (theta, gamma)
    cost: float
    index: int

    @classmethod
    def from_record(cls, rec: np.ndarray, N: int) -> "StepResult":      # rec = [J*, k*, u(3), (theta, gamma)_0..N]
        return cls(rec[2:5].copy(), rec[5:].reshape(N + 1, 2).copy(), float(rec[0]), int(rec[1]))


class Engine:
    def __init__(self, cfg: Optional[MPCConfig] = None, model: Optional[DynamicsModel] = None, **overrides):
        self.lib = load_library()
        self.cfg = cfg or MPCConfig()
        for k, v in overrides.items():
            if not hasattr(self.cfg, k):
                raise TypeError(f"unknown config field {k!r}")
            setattr(self.cfg, k, v)
        self._h = C.c_void_p()
        self.has_comm = False          # rovmpc_comm_init has been called: steps of the closed-loop driver are the sharded ones
        c = self.cfg.to_c()
        rc = self.lib.rovmpc_create(C.byref(c), C.byref(self._h))
        if rc != 0:
            msg = self.lib.rovmpc_last_error(None)
            raise RovmpcError(rc, msg.decode() if msg else "")
        self.model = None
        self.set_model(model or default_model())

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.rovmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        check(self.lib, self._h, rc)

    # -- model -----------------------------------------------------------------------------
    def set_model(self, model: DynamicsModel):
        ct = np.asarray(model.prog_theta.code, dtype=np.int32)
        cg = np.asarray(model.prog_gamma.code, dtype=np.int32)
        cs = np.asarray(model.consts if model.consts else [0.0], dtype=np.float64)
        self._check(self.lib.rovmpc_set_model(self._h, model.n_features, _ptr(model.mean), _ptr(model.scale),
                                              _ptr(ct), len(ct), _ptr(cg), len(cg), _ptr(cs), len(model.consts)))
        self.model = model
        note = self.lib.rovmpc_last_error(self._h)
        self.model_note = note.decode() if note else ""     # e.g. why hiprtc specialisation was not used

    @property
    def model_path(self) -> str:
        """'builtin' (compiled-in reference rows), 'interpreter' or 'jit' (hiprtc-specialised)."""
        return ("builtin", "interpreter", "jit")[int(self.lib.rovmpc_model_path(self._h))]

    @property
    def model_structure(self) -> set:
        """What the code generator found in the loaded rows: {"gamma_invariant"} when dgamma/dt reads only (gamma, gamma_prev)
        -- the gamma path is then integrated once per workgroup --, {"theta_stage_free"} when dtheta/dt reads no stage state."""
        b = int(self.lib.rovmpc_model_structure(self._h))
        return {n for k, n in ((1, "gamma_invariant"), (2, "theta_stage_free")) if b & k}

    def set_rotation_table(self, R):
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.shape != (self.cfg.N, 3, 3):
            raise ValueError(f"R must have shape ({self.cfg.N}, 3, 3)")
        self._check(self.lib.rovmpc_set_rotation_table(self._h, _ptr(R)))

    # -- hot path, host buffers ------------------------------------------------------------
    def _U(self, U) -> np.ndarray:
        U = np.ascontiguousarray(U, dtype=self.cfg.np_dtype)
        if U.shape != (self.cfg.K, self.cfg.N, 3):
            raise ValueError(f"U must have shape ({self.cfg.K}, {self.cfg.N}, 3), got {U.shape}")
        return U

    def step(self, state, U) -> StepResult:
        sa = state_array(state)
        U = self._U(U)
        u = np.empty(3); traj = np.empty((self.cfg.N + 1, 2))
        cost = C.c_double(); idx = C.c_int64()
        s = _c_state(sa)
        self._check(self.lib.rovmpc_step(self._h, C.byref(s), _ptr(U), _ptr(u), _ptr(traj), C.byref(cost), C.byref(idx)))
        return StepResult(u, traj, cost.value, idx.value)

    def mpc_step_sampled(self, state, seed: int, step: int, mean, std, warm_start: bool = True) -> np.ndarray:
        """One control step with the candidates drawn on the GPU (Philox4x32-10 keyed by (seed, step), Box-Muller):
        returns the record [J*, k*, u(3), (theta, gamma)_0..N].  One library call; the host sends the state, spins on the
        completion word and reads the record from mapped memory."""
        if getattr(self, "_samp", None) is None:
            self._samp = {"state": State(), "rec": np.empty(self.result_len), "mean": np.empty(3), "std": np.empty(3)}
            self._samp["prec"] = _ptr(self._samp["rec"]); self._samp["pm"] = _ptr(self._samp["mean"]); self._samp["ps"] = _ptr(self._samp["std"])
            self._samp["pstate"] = C.byref(self._samp["state"])
        sp = self._samp
        sa = state if (isinstance(state, np.ndarray) and state.dtype == np.float64 and state.shape == (16,) and state.flags.c_contiguous) else state_array(state)
        C.memmove(sp["pstate"], sa.ctypes.data, 128)
        sp["mean"][:] = mean; sp["std"][:] = std
        rc = self.lib.rovmpc_mpc_step_sampled(self._h, sp["pstate"], seed, step, sp["pm"], sp["ps"], int(warm_start), sp["prec"])
        if rc:
            self._check(rc)
        return sp["rec"]

    # -- MPPI (rovmpc_mppi_*) and CEM (rovmpc_cem_*) -----------------------------------------------
    def _plan_reset(self, fn, plan, name: str):
        plan = np.ascontiguousarray(plan, dtype=np.float64)
        if plan.shape != (self.cfg.N, 3):
            raise ValueError(f"{name} must have shape ({self.cfg.N}, 3), got {plan.shape}")
        self._check(fn(self._h, _ptr(plan)))

    def _plan_last(self, fn):
        U, J = np.empty((self.cfg.K, self.cfg.N, 3), dtype=self.cfg.np_dtype), np.empty(self.cfg.K, dtype=self.cfg.np_dtype)
        self._check(fn(self._h, _ptr(U), _ptr(J)))
        return U, J

    @staticmethod
    def _triple(v, name: str):
        """None, or (3,) float64 as it is (the library checks the values)."""
        if v is None:
            return None
        a = np.ascontiguousarray(v, dtype=np.float64)
        if a.shape != (3,):
            raise ValueError(f"{name} must have shape (3,), got {a.shape}")
        return a

    def set_noise_correlation(self, beta=None):
        """AR(1) coefficient per control channel of the MPPI / CEM sampling noise along the horizon (rovmpc_set_noise_correlation):
        3 finite values in [0, 1); None or zeros: white noise, the default.  Holds from the next control step, for every
        MPPI and CEM entry of this engine."""
        self._check(self.lib.rovmpc_set_noise_correlation(self._h, _ptr(self._triple(beta, "beta"))))

    def mppi_set_bounds(self, lo=None, hi=None):
        """Box on the MPPI controls (rovmpc_mppi_set_bounds): candidates, nominal and the returned control are clamped to
        [lo, hi] per channel (+-inf allowed); both None: unbounded, the default.  Holds from the next control step."""
        self._check(self.lib.rovmpc_mppi_set_bounds(self._h, _ptr(self._triple(lo, "lo")), _ptr(self._triple(hi, "hi"))))

    def set_nav_cost(self, nav=None, tracks=None):
        """The navigation cost of every MPPI and CEM entry of this engine (rovmpc_set_nav_cost): ``nav`` a ``_lib.NavCost`` and
        ``tracks`` (Bt, Tr, 3) float64, both as ``_lib.nav_cost(...)`` returns them; ``nav`` None: clear.  Holds from the next
        control step."""
        if nav is None:
            self._check(self.lib.rovmpc_set_nav_cost(self._h, None, None, 0, 0))
            return
        if not isinstance(nav, _lib.NavCost):
            raise TypeError("nav must be a _lib.NavCost (_lib.nav_cost(...))")
        tr = np.ascontiguousarray(tracks, dtype=np.float64)
        if tr.ndim != 3 or tr.shape[2] != 3:
            raise ValueError(f"tracks must have shape (Bt, Tr, 3), got {tr.shape}")
        self._check(self.lib.rovmpc_set_nav_cost(self._h, C.byref(nav), _ptr(tr), tr.shape[0], tr.shape[1]))

    def nav_cost(self, state, U, step: int, J=None):
        """C (K,) float64 of the navigation cost alone for candidates U (K, N, 3) at control step ``step`` on track 0, through
        the device entry (rovmpc_nav_cost_device).  With ``J`` (K,), also J' of the law: returns (C, J')."""
        import torch
        dev = torch.device("cuda", self.cfg.device)
        d_state = torch.tensor(state_array(state), device=dev)
        d_U = torch.tensor(self._U(U), device=dev)
        d_C = torch.empty(self.cfg.K, dtype=torch.float64, device=dev)
        d_J = None
        if J is not None:
            Jh = np.ascontiguousarray(J, dtype=self.cfg.np_dtype)
            if Jh.shape != (self.cfg.K,):
                raise ValueError(f"J must have shape ({self.cfg.K},), got {Jh.shape}")
            d_J = torch.tensor(Jh, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_nav_cost_device(self._h, d_state.data_ptr(), d_U.data_ptr(), int(step) & 0xFFFFFFFFFFFFFFFF,
                                                    d_C.data_ptr(), d_J.data_ptr() if d_J is not None else None,
                                                    torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        C_out = d_C.cpu().numpy()
        return C_out if d_J is None else (C_out, d_J.cpu().numpy())

    def set_tether_cost(self, tether=None):
        """The tether keep-out cost of every MPPI and CEM entry of this engine (rovmpc_set_tether_cost): ``tether`` a
        ``_lib.TetherCost`` as ``_lib.tether_cost(...)`` returns it; None: clear.  Holds from the next control step."""
        if tether is None:
            self._check(self.lib.rovmpc_set_tether_cost(self._h, None))
            return
        if not isinstance(tether, _lib.TetherCost):
            raise TypeError("tether must be a _lib.TetherCost (_lib.tether_cost(...))")
        self._check(self.lib.rovmpc_set_tether_cost(self._h, C.byref(tether)))

    def tether_cost(self, state, U, traj, J=None):
        """(C (K,), D (K, N)) float64 of the tether cost alone for candidates U (K, N, 3) whose rollout stored the angles
        ``traj`` (K, N + 1, 2), through the device entry (rovmpc_tether_cost_device): C_k of the law and the signed clearance
        of every node's cable from the nearest sphere surface grown by the margin (NaN at a non-finite node).  With ``J``
        (K,), also J' of the law: returns (C, D, J')."""
        import torch
        dev = torch.device("cuda", self.cfg.device)
        K, N = self.cfg.K, self.cfg.N
        tr = np.ascontiguousarray(traj, dtype=self.cfg.np_dtype)
        if tr.shape != (K, N + 1, 2):
            raise ValueError(f"traj must have shape ({K}, {N + 1}, 2), got {tr.shape}")
        d_state = torch.tensor(state_array(state), device=dev)
        d_U = torch.tensor(self._U(U), device=dev)
        d_traj = torch.tensor(tr, device=dev)
        d_C = torch.empty(K, dtype=torch.float64, device=dev)
        d_D = torch.empty((K, N), dtype=torch.float64, device=dev)
        d_J = None
        if J is not None:
            Jh = np.ascontiguousarray(J, dtype=self.cfg.np_dtype)
            if Jh.shape != (K,):
                raise ValueError(f"J must have shape ({K},), got {Jh.shape}")
            d_J = torch.tensor(Jh, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_tether_cost_device(self._h, d_state.data_ptr(), d_U.data_ptr(), d_traj.data_ptr(),
                                                       d_C.data_ptr(), d_D.data_ptr(), d_J.data_ptr() if d_J is not None else None,
                                                       torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        out = (d_C.cpu().numpy(), d_D.cpu().numpy())
        return out if d_J is None else out + (d_J.cpu().numpy(),)

    def mppi_reset(self, nominal):
        """Set the handle's MPPI nominal plan (N, 3); allocates the MPPI buffers on first use."""
        self._plan_reset(self.lib.rovmpc_mppi_reset, nominal, "nominal")

    def mppi_step(self, state, seed: int, step: int, params: MPPIParams):
        """One MPPI control step: returns (record [J*, k*, u(3), traj], nu* (N, 3), stats (rho, eta, ESS, J_0))."""
        if not isinstance(params, MPPIParams):
            raise TypeError("params must be an MPPIParams (MPPIParams.make(...))")
        s = _c_state(state_array(state))
        rec = np.empty(self.result_len); nu = np.empty((self.cfg.N, 3)); stats = np.empty(4)
        self._check(self.lib.rovmpc_mppi_step(self._h, C.byref(s), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                              C.byref(params), _ptr(rec), _ptr(nu), _ptr(stats)))
        return rec, nu, stats

    def mppi_last(self):
        """Host copies of the last MPPI iteration's candidates U (K, N, 3) and costs J (K,)."""
        return self._plan_last(self.lib.rovmpc_mppi_last)

    def mppi_update_device(self, d_J: int, d_U: int, lam: float, d_nominal_in: int, d_nominal_out: int, d_stats: int = 0,
                           stream: int = 0):
        """The weighted update alone on device buffers (raw pointers), asynchronous on `stream`."""
        self._check(self.lib.rovmpc_mppi_update_device(self._h, d_J, d_U, float(lam), d_nominal_in, d_nominal_out,
                                                       d_stats or None, stream))

    def cem_reset(self, mean):
        """Set the handle's CEM mean (N, 3); allocates the CEM buffers on first use."""
        self._plan_reset(self.lib.rovmpc_cem_reset, mean, "mean")

    def cem_step(self, state, seed: int, step: int, params: CEMParams):
        """One CEM control step: returns (record [J*, k*, u(3), traj], mu* (N, 3), sigma* (N, 3), elites (n_elite,) int64,
        stats (J rank 0, J rank E'-1, |F|, J_0))."""
        if not isinstance(params, CEMParams):
            raise TypeError("params must be a CEMParams (CEMParams.make(...))")
        s = _c_state(state_array(state))
        rec = np.empty(self.result_len); mu = np.empty((self.cfg.N, 3)); sg = np.empty((self.cfg.N, 3))
        el = np.empty(params.n_elite, dtype=np.int64); stats = np.empty(4)
        self._check(self.lib.rovmpc_cem_step(self._h, C.byref(s), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                             C.byref(params), _ptr(rec), _ptr(mu), _ptr(sg), _ptr(el), _ptr(stats)))
        return rec, mu, sg, el, stats

    def cem_last(self):
        """Host copies of the last CEM iteration's candidates U (K, N, 3) and costs J (K,)."""
        return self._plan_last(self.lib.rovmpc_cem_last)

    def cem_update_device(self, d_J: int, d_U: int, params: CEMParams, d_mean_in: int, d_std_in: int, d_mean_out: int,
                          d_std_out: int, d_elite_out: int = 0, d_stats: int = 0, stream: int = 0):
        """The elite selection and refit alone on device buffers (raw pointers), asynchronous on `stream`."""
        if not isinstance(params, CEMParams):
            raise TypeError("params must be a CEMParams (CEMParams.make(...))")
        self._check(self.lib.rovmpc_cem_update_device(self._h, d_J, d_U, C.byref(params), d_mean_in, d_std_in, d_mean_out,
                                                      d_std_out, d_elite_out or None, d_stats or None, stream))

    # -- batched MPPI / CEM (rovmpc_*_batch): B plans advanced by one library call -----------------------
    def _batch_inputs(self, B: int, states, seeds):
        st = np.ascontiguousarray(states, dtype=np.float64)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if st.shape != (B, 16):
            raise ValueError(f"states must have shape ({B}, 16), got {st.shape}")
        if sd.shape != (B,):
            raise ValueError(f"seeds must have shape ({B},), got {sd.shape}")
        return st, sd

    def _plan_reset_batch(self, fn, plans, name: str) -> int:
        plans = np.ascontiguousarray(plans, dtype=np.float64)
        if plans.ndim != 3 or plans.shape[1:] != (self.cfg.N, 3):
            raise ValueError(f"{name} must have shape (B, {self.cfg.N}, 3), got {plans.shape}")
        self._check(fn(self._h, plans.shape[0], _ptr(plans)))
        return plans.shape[0]

    def _plan_last_batch(self, fn, B: Optional[int], known: int, name: str):
        # The library copies its own B problems whatever the caller believes: the arrays are sized from the B of this
        # engine's last successful reset or step, and a caller that reset through the raw library says so with `B`.
        if B is None:
            B = known
        if isinstance(B, bool) or int(B) != B or not 1 <= int(B) <= 1024 or (known and int(B) != known):
            raise ValueError(f"{name}: B = {B!r}, but this engine's batch has {known} problems (0: no reset_batch yet)")
        B = int(B)
        U = np.empty((B, self.cfg.K, self.cfg.N, 3), dtype=self.cfg.np_dtype)
        J = np.empty((B, self.cfg.K), dtype=self.cfg.np_dtype)
        self._check(fn(self._h, _ptr(U), _ptr(J)))
        return U, J

    def mppi_reset_batch(self, nominals):
        """Set the B nominal plans (B, N, 3) of the batched MPPI; (re)allocates its buffers when B changes."""
        self._mppi_B = self._plan_reset_batch(self.lib.rovmpc_mppi_reset_batch, nominals, "nominals")

    def mppi_step_batch(self, states, seeds, step: int, params: MPPIParams):
        """One MPPI control step of B problems (states (B, 16), seeds (B,)): returns (records (B, result_len),
        nu* (B, N, 3), stats (B, 4)); problem b's are bit for bit those of ``mppi_step`` on its own."""
        if not isinstance(params, MPPIParams):
            raise TypeError("params must be an MPPIParams (MPPIParams.make(...))")
        B = len(seeds)
        st, sd = self._batch_inputs(B, states, seeds)
        rec = np.empty((B, self.result_len)); nu = np.empty((B, self.cfg.N, 3)); stats = np.empty((B, 4))
        self._check(self.lib.rovmpc_mppi_step_batch(self._h, B, _ptr(st), _ptr(sd), int(step) & 0xFFFFFFFFFFFFFFFF, C.byref(params),
                                                    _ptr(rec), _ptr(nu), _ptr(stats)))
        self._mppi_B = B                 # the library took the step, so its batch has B problems
        return rec, nu, stats

    def mppi_last_batch(self, B: Optional[int] = None):
        """Host copies of the last batched MPPI iteration's candidates U (B, K, N, 3) and costs J (B, K)."""
        return self._plan_last_batch(self.lib.rovmpc_mppi_last_batch, B, getattr(self, "_mppi_B", 0), "mppi_last_batch")

    def cem_reset_batch(self, means):
        """Set the B mean plans (B, N, 3) of the batched CEM; (re)allocates its buffers when B changes."""
        self._cem_B = self._plan_reset_batch(self.lib.rovmpc_cem_reset_batch, means, "means")

    def cem_step_batch(self, states, seeds, step: int, params: CEMParams):
        """One CEM control step of B problems: returns (records (B, result_len), mu* (B, N, 3), sigma* (B, N, 3),
        elites (B, n_elite) int64, stats (B, 4)); problem b's are bit for bit those of ``cem_step`` on its own."""
        if not isinstance(params, CEMParams):
            raise TypeError("params must be a CEMParams (CEMParams.make(...))")
        B = len(seeds)
        st, sd = self._batch_inputs(B, states, seeds)
        rec = np.empty((B, self.result_len)); mu = np.empty((B, self.cfg.N, 3)); sg = np.empty((B, self.cfg.N, 3))
        el = np.empty((B, params.n_elite), dtype=np.int64); stats = np.empty((B, 4))
        self._check(self.lib.rovmpc_cem_step_batch(self._h, B, _ptr(st), _ptr(sd), int(step) & 0xFFFFFFFFFFFFFFFF, C.byref(params),
                                                   _ptr(rec), _ptr(mu), _ptr(sg), _ptr(el), _ptr(stats)))
        self._cem_B = B                  # the library took the step, so its batch has B problems
        return rec, mu, sg, el, stats

    def cem_last_batch(self, B: Optional[int] = None):
        """Host copies of the last batched CEM iteration's candidates U (B, K, N, 3) and costs J (B, K)."""
        return self._plan_last_batch(self.lib.rovmpc_cem_last_batch, B, getattr(self, "_cem_B", 0), "cem_last_batch")

    # -- device-resident closed loops of MPPI / CEM (rovmpc_*_closed_loop*_device): raw device pointers --------------
    def mppi_row_len(self) -> int:
        """Doubles per control step in the rows of the MPPI loops: [record, nu* (N x 3), stats (4)]."""
        return int(self.lib.rovmpc_mppi_row_len(self._h))

    def cem_row_len(self, n_elite: int) -> int:
        """64-bit words per control step in the rows of the CEM loops: [record, mu*, sigma*, stats (4), elites (n_elite, int64)]."""
        return int(self.lib.rovmpc_cem_row_len(self._h, int(n_elite)))

    def mppi_closed_loop_device(self, d_exo: int, T: int, feedback: bool, seed: int, step0: int, params: MPPIParams, d_rows: int):
        """T MPPI control steps by one call: d_exo[T][16] measured rows, d_rows[T][mppi_row_len] (device memory); blocks once."""
        if not isinstance(params, MPPIParams):
            raise TypeError("params must be an MPPIParams (MPPIParams.make(...))")
        self._check(self.lib.rovmpc_mppi_closed_loop_device(self._h, d_exo, int(T), int(feedback), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                            int(step0) & 0xFFFFFFFFFFFFFFFF, C.byref(params), d_rows))

    def cem_closed_loop_device(self, d_exo: int, T: int, feedback: bool, seed: int, step0: int, params: CEMParams, d_rows: int):
        """T CEM control steps by one call: d_exo[T][16], d_rows[T][cem_row_len(params.n_elite)] (device memory); blocks once."""
        if not isinstance(params, CEMParams):
            raise TypeError("params must be a CEMParams (CEMParams.make(...))")
        self._check(self.lib.rovmpc_cem_closed_loop_device(self._h, d_exo, int(T), int(feedback), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                           int(step0) & 0xFFFFFFFFFFFFFFFF, C.byref(params), d_rows))

    def mppi_closed_loop_batch_device(self, d_exo: int, T: int, feedback: bool, seeds, step0: int, params: MPPIParams, d_rows: int):
        """The same for the batch of B = len(seeds) problems: d_exo[B][T][16], d_rows[T][B][mppi_row_len]."""
        if not isinstance(params, MPPIParams):
            raise TypeError("params must be an MPPIParams (MPPIParams.make(...))")
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        self._check(self.lib.rovmpc_mppi_closed_loop_batch_device(self._h, len(sd), d_exo, int(T), int(feedback), _ptr(sd),
                                                                  int(step0) & 0xFFFFFFFFFFFFFFFF, C.byref(params), d_rows))
        self._mppi_B = len(sd)

    def cem_closed_loop_batch_device(self, d_exo: int, T: int, feedback: bool, seeds, step0: int, params: CEMParams, d_rows: int):
        """The same for the batch of B = len(seeds) problems: d_exo[B][T][16], d_rows[T][B][cem_row_len(params.n_elite)]."""
        if not isinstance(params, CEMParams):
            raise TypeError("params must be a CEMParams (CEMParams.make(...))")
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        self._check(self.lib.rovmpc_cem_closed_loop_batch_device(self._h, len(sd), d_exo, int(T), int(feedback), _ptr(sd),
                                                                 int(step0) & 0xFFFFFFFFFFFFFFFF, C.byref(params), d_rows))
        self._cem_B = len(sd)

    def sampled_candidates(self) -> np.ndarray:
        """Host copy of the candidate tensor of the last ``mpc_step_sampled`` (tests / inspection)."""
        U = np.empty((self.cfg.K, self.cfg.N, 3), dtype=self.cfg.np_dtype)
        self._check(self.lib.rovmpc_sampled_candidates(self._h, _ptr(U)))
        return U

    def sample_candidates_device(self, seed: int, step: int, mean, std, d_U: int, stream: int = 0):
        m = np.ascontiguousarray(mean, np.float64); s = np.ascontiguousarray(std, np.float64)
        self._check(self.lib.rovmpc_sample_candidates_device(self._h, seed, step, _ptr(m), _ptr(s), d_U, stream))

    def rollout_costs(self, state, U, return_traj: bool = False):
        sa = state_array(state)
        U = self._U(U)
        J = np.empty(self.cfg.K, dtype=self.cfg.np_dtype)
        traj = np.empty((self.cfg.K, self.cfg.N + 1, 2), dtype=self.cfg.np_dtype) if return_traj else None
        s = _c_state(sa)
        self._check(self.lib.rovmpc_rollout_costs(self._h, C.byref(s), _ptr(U), _ptr(J), _ptr(traj)))
        return (J, traj) if return_traj else J

    # -- hot path, device buffers (raw pointers; torch tensors' data_ptr()) ----------------
    @property
    def result_len(self) -> int:
        return int(self.lib.rovmpc_result_len(self._h))

    def step_device(self, d_state: int, d_U: int, d_result: int, stream: int = 0):
        self._check(self.lib.rovmpc_step_device(self._h, d_state, d_U, d_result, stream))

    def step_device_sharded(self, d_state: int, d_U: int, k_offset: int, rank: int, world: int, d_slots: int,
                            stream: int = 0):
        self._check(self.lib.rovmpc_step_device_sharded(self._h, d_state, d_U, k_offset, rank, world, d_slots, stream))

    def select_device(self, d_slots: int, world: int, d_result: int, stream: int = 0):
        self._check(self.lib.rovmpc_select_device(self._h, d_slots, world, d_result, stream))

    # -- native collective (RCCL called from the library) -----------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        rc = self.lib.rovmpc_comm_unique_id(buf)
        if rc != 0:
            msg = self.lib.rovmpc_last_error(None)
            raise RovmpcError(rc, msg.decode() if msg else "")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be 128 bytes")
        self._check(self.lib.rovmpc_comm_init(self._h, C.create_string_buffer(unique_id, 128), rank, world))
        self.has_comm = True

    def step_device_allreduce(self, d_state: int, d_U: int, k_offset: int, d_result: int, stream: int = 0):
        self._check(self.lib.rovmpc_step_device_allreduce(self._h, d_state, d_U, k_offset, d_result, stream))

    def comm_join(self, stream: int = 0):
        self._check(self.lib.rovmpc_comm_join(self._h, stream))

    def comm_sync(self, stream: int = 0):
        """Join + synchronise ``stream``; raises ``RovmpcError`` if a GPU-side hand-off of any enqueued step gave up."""
        self._check(self.lib.rovmpc_comm_sync(self._h, stream))

    def comm_abort(self):
        """ncclCommAbort on the handle's communicators (callable from another thread while a synchronise is stuck)."""
        self._check(self.lib.rovmpc_comm_abort(self._h))

    def comm_placement(self) -> str:
        """One-line report of the collective-stream placement probe (empty before the first sharded step)."""
        v = self.lib.rovmpc_comm_placement(self._h)
        return v.decode() if v else ""

    def set_option(self, name: str, value: float):
        self._check(self.lib.rovmpc_set_option(self._h, name.encode(), float(value)))

    def device_status(self):
        self._check(self.lib.rovmpc_device_status(self._h))

    def step_batch_device(self, B: int, d_states: int, d_U: int, d_results: int, stream: int = 0):
        """B independent problems in one launch: d_states[B][16], d_U[B][K][N][3], d_results[B][result_len]."""
        self._check(self.lib.rovmpc_step_batch_device(self._h, B, d_states, d_U, d_results, stream))

    def batch_costs_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self.lib.rovmpc_batch_costs_device(self._h, C.byref(p)))
        return p.value

    def comm_destroy(self):
        self.has_comm = False
        self._check(self.lib.rovmpc_comm_destroy(self._h))

    def closed_loop_device(self, d_exo: int, T: int, d_state: int, d_pools: int, n_pools: int, d_results: int,
                           k_offset: int = 0, feedback: bool = False, stream: int = 0, mode: str = ""):
        """mode: "per_step" (one launch per step, one stream; also the sharded loop) or "pipelined" (one launch per step,
        two streams, GPU-side state hand-off; single GPU)."""
        mode = mode or "per_step"
        if mode == "pipelined":
            if k_offset:
                raise ValueError("the pipelined loop is single-GPU (k_offset must be 0)")
            self._check(self.lib.rovmpc_closed_loop_pipelined_device(self._h, d_exo, T, d_state, d_pools, n_pools, int(feedback),
                                                                     d_results, stream))
            return
        if mode != "per_step":
            raise ValueError(f"unknown closed-loop mode {mode!r}")
        self._check(self.lib.rovmpc_closed_loop_device(self._h, d_exo, T, d_state, d_pools, n_pools, k_offset,
                                                       int(feedback), d_results, stream))

    @property
    def closed_loop_form(self) -> str:
        """Form the last ``closed_loop_device`` call took: "none" (none yet, or refused), "per_step" (single GPU, one launch
        per step), "pipelined", "sharded_join" (a join per step) or "sharded_handoff" (state handed over on the GPU)."""
        return ("none", "per_step", "pipelined", "sharded_join", "sharded_handoff")[int(self.lib.rovmpc_closed_loop_form(self._h))]

    def timing_enable(self, max_launches: int):
        self._check(self.lib.rovmpc_timing_enable(self._h, max_launches))

    def timing_read(self):
        avg = C.c_double(); mn = C.c_double(); n = C.c_int32()
        self._check(self.lib.rovmpc_timing_read(self._h, C.byref(avg), C.byref(mn), C.byref(n)))
        return avg.value, mn.value, n.value

    def math_probe(self, fn, x, y=None, dtype: str = "f64"):
        """Diagnostic (``rovmpc_math_probe``): the device math primitive ``fn`` (a name of ``_lib.PROBE_FN``) on every element
        of x (and y, for the two-operand ones); element i runs on global thread i of 256-thread blocks.  ``dtype`` "f64" or
        "f32" (inputs converted with a plain float32 cast, results widened).  Returns one float64 array, or (sin, cos) for the pairs."""
        if fn not in _lib.PROBE_FN:
            raise ValueError(f"unknown probe function {fn!r}")
        if dtype not in ("f64", "f32"):
            raise ValueError(f"dtype must be 'f64' or 'f32' (got {dtype!r})")
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if (y is not None) != (fn in _lib.PROBE_TWO_OPERANDS):
            raise ValueError(f"{fn} takes {'two operands' if fn in _lib.PROBE_TWO_OPERANDS else 'one operand'}")
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
            if y.shape != x.shape:
                raise ValueError("x and y must have the same length")
        out0 = np.empty(x.shape[0])
        out1 = np.empty(x.shape[0]) if fn in _lib.PROBE_TWO_RESULTS else None
        self._check(self.lib.rovmpc_math_probe(self._h, _lib.PROBE_FN[fn], _lib.F32 if dtype == "f32" else _lib.F64, _ptr(x), _ptr(y),
                                               x.shape[0], _ptr(out0), _ptr(out1)))
        return out0 if out1 is None else (out0, out1)

    # -- batched helper mirrors ------------------------------------------------------------
    def predict(self, Xs, which: int) -> np.ndarray:
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.model.n_features:
            raise ValueError(f"X must be (n, {self.model.n_features})")
        out = np.empty(Xs.shape[0])
        self._check(self.lib.rovmpc_predict(self._h, _ptr(Xs), Xs.shape[0], which, _ptr(out)))
        return out

    def eval_expression(self, code, consts, X) -> np.ndarray:
        """A compiled expression (``expr.compile_expression``) on every row of X (n, F)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be (n, F)")
        c = np.asarray(code, dtype=np.int32); k = np.asarray(consts if len(consts) else [0.0], dtype=np.float64)
        out = np.empty(X.shape[0])
        self._check(self.lib.rovmpc_eval_expression(self._h, _ptr(c), len(c), _ptr(k), len(consts), _ptr(X), X.shape[1], X.shape[0], _ptr(out)))
        return out

    def lagrangian_rollout(self, code_theta, code_gamma, consts, time, y0):
        """evaluate_lagrangian_on_test.py:59-68 for B initial states y0 (B, 4) = (theta, gamma, vtheta, vgamma): four (B, T) arrays."""
        time = np.ascontiguousarray(time, dtype=np.float64).reshape(-1)
        y0 = np.ascontiguousarray(y0, dtype=np.float64).reshape(-1, 4)
        ct = np.asarray(code_theta, dtype=np.int32); cg = np.asarray(code_gamma, dtype=np.int32)
        k = np.asarray(consts if len(consts) else [0.0], dtype=np.float64)
        out = np.empty((4, y0.shape[0], time.shape[0]))
        self._check(self.lib.rovmpc_lagrangian_rollout(self._h, _ptr(ct), len(ct), _ptr(cg), len(cg), _ptr(k), len(consts), _ptr(time),
                                                       time.shape[0], _ptr(y0), y0.shape[0], _ptr(out)))
        return out[0], out[1], out[2], out[3]

    def replay(self, Xs, time, theta0: float, gamma0: float, integrator: int = _lib.RK4):
        Xs = np.ascontiguousarray(Xs, dtype=np.float64); time = np.ascontiguousarray(time, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.model.n_features or time.shape != (Xs.shape[0],):
            raise ValueError("x_input must be (T, n_features) and time (T,)")
        th = np.empty(len(time)); ga = np.empty(len(time))
        self._check(self.lib.rovmpc_replay(self._h, _ptr(Xs), _ptr(time), len(time), float(theta0), float(gamma0),
                                           integrator, _ptr(th), _ptr(ga)))
        return th, ga

    def solve_catenary(self, l, delta_H, L: float, with_tension: bool = False):
        l, dH = np.broadcast_arrays(np.asarray(l, np.float64), np.asarray(delta_H, np.float64))
        shape = l.shape
        l = np.ascontiguousarray(l).reshape(-1); dH = np.ascontiguousarray(dH).reshape(-1)
        Cc = np.empty(l.size); T = np.empty(l.size) if with_tension else None
        self._check(self.lib.rovmpc_solve_catenary(self._h, _ptr(l), _ptr(dH), float(L), l.size, _ptr(Cc), _ptr(T)))
        return (Cc.reshape(shape), T.reshape(shape)) if with_tension else Cc.reshape(shape)

    def rodrigues(self, v, axis, angle) -> np.ndarray:
        v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
        axis = np.ascontiguousarray(np.broadcast_to(np.asarray(axis, np.float64), v.shape))
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, np.float64), (v.shape[0],)))
        out = np.empty_like(v)
        self._check(self.lib.rovmpc_rodrigues(self._h, _ptr(v), _ptr(axis), _ptr(angle), v.shape[0], _ptr(out)))
        return out

    def catenary_points(self, A, B, L: float, M: int):
        A = np.ascontiguousarray(A, np.float64).reshape(-1, 3); B = np.ascontiguousarray(B, np.float64).reshape(-1, 3)
        n = A.shape[0]
        pts = np.empty((n, M, 3)); valid = np.empty(n, np.int32); params = np.empty((n, 3))
        self._check(self.lib.rovmpc_catenary_points(self._h, _ptr(A), _ptr(B), float(L), n, M, _ptr(pts), _ptr(valid),
                                                    _ptr(params)))
        return pts, valid.astype(bool), params

    def compute_catenary_3d(self, p0, p1, rope_length: float, num_points: int):
        """models/catenary_3d.py:5-39 for n pairs: (pts (n, num_points, 3), a (n,)); a = NaN where the rope is taut."""
        A = np.ascontiguousarray(p0, np.float64).reshape(-1, 3); B = np.ascontiguousarray(p1, np.float64).reshape(-1, 3)
        if A.shape != B.shape:
            raise ValueError("p0 and p1 must have the same shape")
        if num_points < 2:
            raise ValueError("num_points must be >= 2")
        n = A.shape[0]
        pts = np.empty((n, num_points, 3)); a = np.empty(n)
        self._check(self.lib.rovmpc_compute_catenary_3d(self._h, _ptr(A), _ptr(B), float(rope_length), n, int(num_points),
                                                        _ptr(pts), _ptr(a)))
        return pts, a

    def transform_catenary(self, A, B, theta, gamma, L: float, M: int):
        A = np.ascontiguousarray(A, np.float64).reshape(-1, 3); B = np.ascontiguousarray(B, np.float64).reshape(-1, 3)
        n = A.shape[0]
        th = np.ascontiguousarray(np.broadcast_to(np.asarray(theta, np.float64), (n,)))
        ga = np.ascontiguousarray(np.broadcast_to(np.asarray(gamma, np.float64), (n,)))
        out = np.empty((4, n, M, 3)); npts = np.empty((n, 2), np.int32); z = np.empty(n)
        self._check(self.lib.rovmpc_transform_catenary(self._h, _ptr(A), _ptr(B), _ptr(th), _ptr(ga), float(L), n, M,
                                                       _ptr(out), _ptr(npts), _ptr(z)))
        return out, npts, z

    def velocity_transform(self, R, v) -> np.ndarray:
        R = np.ascontiguousarray(R, np.float64).reshape(-1, 3, 3); v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
        if R.shape[0] != v.shape[0]:
            raise ValueError("R and v must have the same number of rows")
        out = np.empty_like(v)
        self._check(self.lib.rovmpc_velocity_transform(self._h, _ptr(R), _ptr(v), v.shape[0], _ptr(out)))
        return out

    def extract_features(self, P0, P1, V1, time, theta, gamma, with_prev: bool = True) -> np.ndarray:
        c = lambda x, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), shape))
        time = np.ascontiguousarray(time, np.float64).reshape(-1)
        T = time.shape[0]
        P0, P1, V1 = c(P0, (T, 3)), c(P1, (T, 3)), c(V1, (T, 3))
        theta, gamma = c(np.asarray(theta, np.float64).reshape(-1), (T,)), c(np.asarray(gamma, np.float64).reshape(-1), (T,))
        out = np.empty((T, 18 if with_prev else 16))
        self._check(self.lib.rovmpc_extract_features(self._h, _ptr(P0), _ptr(P1), _ptr(V1), _ptr(time), _ptr(theta),
                                                     _ptr(gamma), T, int(with_prev), _ptr(out)))
        return out

    def features_dd(self, P0_mm, P1_mm, V_mm, time, theta, gamma, window: int = 11, polyorder: int = 3):
        """main_fun.py:811-871 on arrays as logged (mm, mm/s): returns (features (T,14), targets (T,2))."""
        c = lambda x, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), shape))
        time = np.ascontiguousarray(time, np.float64).reshape(-1)
        T = time.shape[0]
        if T < window:
            raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")   # scipy's message
        P0, P1, V = c(P0_mm, (T, 3)), c(P1_mm, (T, 3)), c(V_mm, (T, 3))
        theta, gamma = c(np.asarray(theta, np.float64).reshape(-1), (T,)), c(np.asarray(gamma, np.float64).reshape(-1), (T,))
        F = np.empty((T, 14)); Y = np.empty((T, 2))
        self._check(self.lib.rovmpc_features_dd(self._h, _ptr(P0), _ptr(P1), _ptr(V), _ptr(time), _ptr(theta), _ptr(gamma),
                                                T, window, polyorder, _ptr(F), _ptr(Y)))
        return F, Y

    def gaussian_filter1d(self, x, sigma: float, truncate: float = 4.0) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        out = np.empty_like(x)
        self._check(self.lib.rovmpc_gaussian_filter1d(self._h, _ptr(x), x.shape[0], float(sigma), float(truncate), _ptr(out)))
        return out

    def kabsch_velocity_transform(self, P, Q, v, batch_gates: bool = True):
        P = np.ascontiguousarray(P, np.float64); Q = np.ascontiguousarray(Q, np.float64)
        v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
        if P.ndim != 3 or P.shape[2] != 3 or Q.shape != P.shape or v.shape[0] != P.shape[0]:
            raise ValueError("P, Q must be (T, M, 3) and v (T, 3)")
        T, M = P.shape[0], P.shape[1]
        out = np.empty((T, 3)); R = np.empty((T, 3, 3))
        self._check(self.lib.rovmpc_kabsch_velocity_transform(self._h, _ptr(P), _ptr(Q), _ptr(v), T, M, int(batch_gates),
                                                              _ptr(out), _ptr(R)))
        return out, R

    def _fit_inputs(self, P0, P1, markers, guess):
        Y = np.ascontiguousarray(markers, np.float64)
        single = Y.ndim == 2
        if single:
            Y = Y[None]
        if Y.ndim != 3 or Y.shape[2] != 3:
            raise ValueError(f"markers must be (M, 3) or (B, M, 3), got {np.shape(markers)}")
        B, M = Y.shape[0], Y.shape[1]
        if not 3 <= M <= _lib.FIT_MAX_MARKERS:
            raise ValueError(f"3 to {_lib.FIT_MAX_MARKERS} markers per frame (got {M})")
        c = lambda x, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), shape))
        P0, P1 = c(P0, (B, 3)), c(P1, (B, 3))
        G = None if guess is None else c(guess, (B, 2))
        return P0, P1, Y, G, B, M, single

    @staticmethod
    def _fit_result(out, single):
        cols = [out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4].astype(np.int64), out[:, 5].astype(np.int64)]
        return CableFit(*[col[0] for col in cols]) if single else CableFit(*cols)

    def fit_theta_gamma(self, P0, P1, markers, guess=None, tol: float = 1e-12, max_iter: int = 40) -> "CableFit":
        """(theta, gamma) of the cable between P0 and P1 from its markers (rovmpc_fit_theta_gamma; law in include/rovmpc.h):
        ``markers`` (M, 3) for one frame or (B, M, 3), 3 <= M <= 16, a NaN row = a missing marker; P0, P1 (3,) or (B, 3);
        ``guess`` (2,) or (B, 2): the start, (0, 0) if None.  A local fit from that start.  Returns a ``CableFit`` of
        arrays (B,), scalars for one frame; ``status`` holds ``FitStatus`` values."""
        P0, P1, Y, G, B, M, single = self._fit_inputs(P0, P1, markers, guess)
        params = FitParams.make(tol, max_iter)
        out = np.empty((B, _lib.FIT_OUT))
        self._check(self.lib.rovmpc_fit_theta_gamma(self._h, _ptr(P0), _ptr(P1), _ptr(Y), B, M, _ptr(G), C.byref(params), _ptr(out)))
        return self._fit_result(out, single)

    def fit_theta_gamma_device(self, P0, P1, markers, guess=None, tol: float = 1e-12, max_iter: int = 40) -> "CableFit":
        """``fit_theta_gamma`` through the device entry (rovmpc_fit_theta_gamma_device) on torch buffers: the same bits."""
        import torch
        dev = torch.device("cuda", self.cfg.device)
        P0, P1, Y, G, B, M, single = self._fit_inputs(P0, P1, markers, guess)
        params = FitParams.make(tol, max_iter)
        d0, d1, dY = (torch.tensor(x, device=dev) for x in (P0, P1, Y))
        dG = None if G is None else torch.tensor(G, device=dev)
        dO = torch.empty((B, _lib.FIT_OUT), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_fit_theta_gamma_device(self._h, d0.data_ptr(), d1.data_ptr(), dY.data_ptr(), B, M,
                                                           None if dG is None else dG.data_ptr(), C.byref(params), dO.data_ptr()))
        torch.cuda.synchronize(dev)                     # (the device: the fit runs on the handle's own stream)
        return self._fit_result(dO.cpu().numpy(), single)

    def calibrate_cable(self, P0, P1, markers, group_off, guess=None, arc=None, L0=None, free_length: bool = True, L_lo: float = 0.0,
                        L_hi: float = float("inf"), tol: float = 1e-12, tol_L: float = 1e-12, max_iter: int = 60, device: bool = False):
        """The cable length of every group of frames (rovmpc_calibrate_cable; law in include/rovmpc.h): P0, P1 (F, 3),
        ``markers`` (F, M, 3), ``group_off`` (G + 1,) offsets, ``guess`` (F, 2) or None, ``arc`` (M,) or None (the index
        rule).  Returns (out_group (G, 8), out_frame (F, 5)) as the entry leaves them; ``rovmpc.calibrate_cable`` shapes the
        arguments and names the columns.  ``device``: through rovmpc_calibrate_cable_device on torch buffers, the same bits."""
        Y = np.ascontiguousarray(markers, np.float64)
        if Y.ndim != 3 or Y.shape[2] != 3:
            raise ValueError(f"markers must be (F, M, 3), got {Y.shape}")
        F, M = Y.shape[:2]
        P0 = np.ascontiguousarray(np.broadcast_to(np.asarray(P0, np.float64), (F, 3)))
        P1 = np.ascontiguousarray(np.broadcast_to(np.asarray(P1, np.float64), (F, 3)))
        G_ = None if guess is None else np.ascontiguousarray(np.broadcast_to(np.asarray(guess, np.float64), (F, 2)))
        off = np.ascontiguousarray(group_off, np.int32)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("group_off must hold G + 1 offsets")
        G = off.size - 1
        s = None if arc is None else np.ascontiguousarray(arc, np.float64)
        if s is not None and s.shape != (M,):
            raise ValueError(f"arc must be ({M},), got {s.shape}")
        params = _lib.CalibParams.make(L0, free_length, L_lo, L_hi, tol, tol_L, max_iter)
        if not device:
            og, of = np.full((G, _lib.CALIB_GROUP_OUT), np.nan), np.full((F, _lib.CALIB_FRAME_OUT), np.nan)
            self._check(self.lib.rovmpc_calibrate_cable(self._h, _ptr(P0), _ptr(P1), _ptr(Y), F, M, _ptr(off), G, _ptr(G_), _ptr(s),
                                                        C.byref(params), _ptr(og), _ptr(of)))
            return og, of
        import torch
        dev = torch.device("cuda", self.cfg.device)
        d0, d1, dY = (torch.tensor(x, device=dev) for x in (P0, P1, Y))
        dG = None if G_ is None else torch.tensor(G_, device=dev)
        dog = torch.full((G, _lib.CALIB_GROUP_OUT), float("nan"), dtype=torch.float64, device=dev)
        dof = torch.full((F, _lib.CALIB_FRAME_OUT), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_calibrate_cable_device(self._h, d0.data_ptr(), d1.data_ptr(), dY.data_ptr(), F, M, _ptr(off), G,
                                                           None if dG is None else dG.data_ptr(), _ptr(s), C.byref(params),
                                                           dog.data_ptr(), dof.data_ptr()))
        torch.cuda.synchronize(dev)                     # (the device: the calibration runs on the handle's own stream)
        return dog.cpu().numpy(), dof.cpu().numpy()

    def cable_markers(self, P0, P1, theta, gamma, L=None, arc=None, M: int = 16) -> np.ndarray:
        """The markers of the cable between P0 and P1 at (theta, gamma) (rovmpc_cable_markers; law in include/rovmpc.h): the
        forward model of ``calibrate_cable``.  theta, gamma scalars or (B,); P0, P1 (3,) or (B, 3); ``L`` None (the
        config's), a scalar or (B,); ``arc`` (M,) fractions of the length from 0 to 1, None = the index rule.  Returns
        (M, 3) for scalars, else (B, M, 3)."""
        th = np.asarray(theta, np.float64)
        single = th.ndim == 0 and np.ndim(gamma) == 0 and np.ndim(P0) == 1 and np.ndim(P1) == 1 and np.ndim(L) == 0
        shape = np.broadcast_shapes(np.shape(theta), np.shape(gamma), np.shape(P0)[:-1], np.shape(P1)[:-1], np.shape(0.0 if L is None else L))
        if len(shape) > 1:
            raise ValueError(f"theta, gamma, L must be scalars or (B,) and P0, P1 (3,) or (B, 3) (got a batch of shape {shape})")
        B = int(shape[0]) if shape else 1
        c = lambda x, sh: np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), sh))
        P0, P1, th, ga = c(P0, (B, 3)), c(P1, (B, 3)), c(theta, (B,)), c(gamma, (B,))
        Lb = None if L is None else c(L, (B,))
        M = int(M)
        s = None if arc is None else np.ascontiguousarray(arc, np.float64)
        if s is not None and s.shape != (M,):
            raise ValueError(f"arc must be ({M},), got {s.shape}")
        out = np.full((B, M, 3), np.nan)
        self._check(self.lib.rovmpc_cable_markers(self._h, _ptr(P0), _ptr(P1), _ptr(th), _ptr(ga), _ptr(Lb), _ptr(s), B, M, _ptr(out)))
        return out[0] if single else out

    def _track_inputs(self, P0, P1, markers, carry):
        Y = np.ascontiguousarray(markers, np.float64)
        single = Y.ndim == 3
        if single:
            Y = Y[None]
        if Y.ndim != 4 or Y.shape[3] != 3:
            raise ValueError(f"markers must be (T, M, 3) or (B, T, M, 3), got {np.shape(markers)}")
        B, T, M = Y.shape[:3]
        if not 3 <= M <= _lib.FIT_MAX_MARKERS:
            raise ValueError(f"3 to {_lib.FIT_MAX_MARKERS} markers per frame (got {M})")
        c = lambda x, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), shape)).copy()
        P0, P1 = c(P0, (B, T, 3)), c(P1, (B, T, 3))
        Cy = None if carry is None else c(carry, (B, 2))
        return P0, P1, Y, Cy, B, T, M, single

    @staticmethod
    def _track_result(out, carry, B, single):
        if carry is None:                               # a fresh start returns no carry: it is the last frame's output angles
            carry = out[:, -1, 0:2].copy() if out.shape[1] else np.full((B, 2), np.nan)
        i = lambda k: out[..., k].astype(np.int64)
        cols = [out[..., 0], out[..., 1], out[..., 2], out[..., 3], out[..., 4], i(5), i(6), i(7), i(8), carry]
        return CableTrack(*[np.ascontiguousarray(col[0] if single else col) for col in cols])

    def track_markers(self, P0, P1, markers, carry=None, starts=None, rms_max: float = float("inf"), tol: float = 1e-12,
                      max_iter: int = 40) -> "CableTrack":
        """(theta, gamma) along a recording (rovmpc_track_markers; law in include/rovmpc.h): ``markers`` (T, M, 3) or
        (B, T, M, 3), a NaN row = a missing marker; P0, P1 (3,), (T, 3) or (B, T, 3); ``carry`` (2,) or (B, 2): the last
        accepted estimate of the call before, None (or NaN) for a fresh start; ``starts``: the re-acquisition list of
        (theta, gamma), the law's default if None; ``rms_max``: accept a converged fit only at or below this rms (metres).
        Returns a ``CableTrack``; ``CableTrack.rows`` fills the state rows the controllers' loops consume."""
        P0, P1, Y, Cy, B, T, M, single = self._track_inputs(P0, P1, markers, carry)
        params = TrackParams.make(starts, rms_max, tol, max_iter)
        out = np.empty((B, T, _lib.TRACK_OUT))
        self._check(self.lib.rovmpc_track_markers(self._h, _ptr(P0), _ptr(P1), _ptr(Y), B, T, M, _ptr(Cy), C.byref(params), _ptr(out)))
        return self._track_result(out, Cy, B, single)

    def track_markers_device(self, P0, P1, markers, carry=None, starts=None, rms_max: float = float("inf"), tol: float = 1e-12,
                             max_iter: int = 40, exo=None):
        """``track_markers`` through the device entry (rovmpc_track_markers_device) on torch buffers: the same bits.  With
        ``exo`` (T, 16) or (B, T, 16) returns (CableTrack, the rows as the entry left them)."""
        import torch
        dev = torch.device("cuda", self.cfg.device)
        P0, P1, Y, Cy, B, T, M, single = self._track_inputs(P0, P1, markers, carry)
        params = TrackParams.make(starts, rms_max, tol, max_iter)
        d0, d1, dY = (torch.tensor(x, device=dev) for x in (P0, P1, Y))
        dC = None if Cy is None else torch.tensor(Cy, device=dev)
        dE = None if exo is None else torch.tensor(np.ascontiguousarray(exo, np.float64).reshape(B, T, 16), device=dev)
        dO = torch.empty((B, T, _lib.TRACK_OUT), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_track_markers_device(self._h, d0.data_ptr(), d1.data_ptr(), dY.data_ptr(), B, T, M,
                                                         None if dC is None else dC.data_ptr(), C.byref(params), dO.data_ptr(),
                                                         None if dE is None else dE.data_ptr()))
        torch.cuda.synchronize(dev)                     # (the device: the tracker runs on the handle's own stream)
        track = self._track_result(dO.cpu().numpy(), None if dC is None else dC.cpu().numpy(), B, single)
        if dE is None:
            return track
        rows = dE.cpu().numpy()
        return track, (rows[0] if single else rows)


    def score_rows(self, programs, X, time, truth, integrator: int = _lib.RK4, target=None, lengths=None, y0=None,
                   return_est: bool = False, return_pred: bool = False, device: bool = False):
        """R compiled rows on B recordings (rovmpc_score_rows; law in include/rovmpc.h).  ``programs``: a sequence of
        (code, consts) per row, each row with its own constants; X (B, T, F), time, truth and target (B, T), lengths and y0
        (B,) or None, checked and laid out by ``scoring.score_rows``.  Returns (scores (R, B, 8), est or None, pred or None).
        ``device=True`` goes through rovmpc_score_rows_device on torch buffers: the same bits."""
        code_off, const_off = [0], [0]
        for code, consts in programs:
            code_off.append(code_off[-1] + len(code)); const_off.append(const_off[-1] + len(consts))
        code = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in programs]), np.int32)
        consts = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float64).reshape(-1) for _, k in programs] + [np.zeros(1)]))
        code_off, const_off = np.asarray(code_off, np.int32), np.asarray(const_off, np.int32)
        R, (B, T, F) = len(programs), X.shape
        lens = None if lengths is None else np.ascontiguousarray(lengths, np.int64)
        shape = (R, B, T)
        if not device:
            scores = np.empty((R, B, _lib.SCORE_COLS))
            est = np.empty(shape) if return_est else None
            pred = np.empty(shape) if return_pred else None
            self._check(self.lib.rovmpc_score_rows(self._h, _ptr(code), _ptr(code_off), _ptr(consts), _ptr(const_off), R, _ptr(X), F,
                                                   _ptr(time), _ptr(lens), T, B, _ptr(truth), _ptr(target), _ptr(y0), int(integrator),
                                                   _ptr(scores), _ptr(est), _ptr(pred)))
            return scores, est, pred
        import torch
        dev = torch.device("cuda", self.cfg.device)
        up = lambda x: None if x is None else torch.tensor(x, device=dev)
        dp = lambda t: None if t is None else t.data_ptr()
        dX, dT, dY, dG, d0 = up(X), up(time), up(truth), up(target), up(y0)
        dS = torch.empty((R, B, _lib.SCORE_COLS), dtype=torch.float64, device=dev)
        dE = torch.empty(shape, dtype=torch.float64, device=dev) if return_est else None
        dP = torch.empty(shape, dtype=torch.float64, device=dev) if return_pred else None
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_score_rows_device(self._h, _ptr(code), _ptr(code_off), _ptr(consts), _ptr(const_off), R, dp(dX), F,
                                                      dp(dT), _ptr(lens), T, B, dp(dY), dp(dG), dp(d0), int(integrator), dp(dS), dp(dE),
                                                      dp(dP)))
        torch.cuda.synchronize(dev)                     # (the device: the scoring runs on the handle's own stream)
        back = lambda t: None if t is None else t.cpu().numpy()
        return back(dS), back(dE), back(dP)

    def refit_rows(self, programs, X, target, lengths=None, group_off=None, free=None, params=None, device: bool = False):
        """The constants of R compiled rows refitted on G groups of recordings (rovmpc_refit_rows; law in include/rovmpc.h).
        ``programs`` as in ``score_rows`` (the constants are the starts); X (B, T, F), target (B, T), lengths (B,) or None,
        group_off int32 (G + 1,) or None (all recordings pooled), free: per row a uint8 mask over its constants, or None (all
        free); params a RefitParams or None, checked and laid out by ``scoring.refit_rows``.  Returns (consts_out (G, NK) with
        NK the constants of all rows, out (R, G, 6)).  ``device=True`` goes through rovmpc_refit_rows_device: the same bits."""
        code_off, const_off = [0], [0]
        for code, consts in programs:
            code_off.append(code_off[-1] + len(code)); const_off.append(const_off[-1] + len(consts))
        code = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in programs]), np.int32)
        consts = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float64).reshape(-1) for _, k in programs] + [np.zeros(1)]))
        mask = None if free is None else np.ascontiguousarray(np.concatenate([np.asarray(m, np.uint8).reshape(-1) for m in free] + [np.zeros(1, np.uint8)]))
        code_off, const_off = np.asarray(code_off, np.int32), np.asarray(const_off, np.int32)
        R, (B, T, F), NK = len(programs), X.shape, int(const_off[-1])
        G = 1 if group_off is None else len(group_off) - 1
        goff = None if group_off is None else np.ascontiguousarray(group_off, np.int32)
        lens = None if lengths is None else np.ascontiguousarray(lengths, np.int64)
        pref = None if params is None else C.byref(params)
        if not device:
            consts_out = np.empty((G, max(NK, 1)))
            out = np.empty((R, G, _lib.REFIT_OUT))
            self._check(self.lib.rovmpc_refit_rows(self._h, _ptr(code), _ptr(code_off), _ptr(consts), _ptr(const_off), _ptr(mask), R, _ptr(X),
                                                   F, _ptr(lens), T, B, _ptr(target), _ptr(goff), G, pref, _ptr(consts_out), _ptr(out)))
            return consts_out.reshape(-1)[:G * NK].reshape(G, NK), out
        import torch
        dev = torch.device("cuda", self.cfg.device)
        dX, dG = torch.tensor(X, device=dev), torch.tensor(target, device=dev)
        dK = torch.empty((G, max(NK, 1)), dtype=torch.float64, device=dev)
        dO = torch.empty((R, G, _lib.REFIT_OUT), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_refit_rows_device(self._h, _ptr(code), _ptr(code_off), _ptr(consts), _ptr(const_off), _ptr(mask), R,
                                                      dX.data_ptr(), F, _ptr(lens), T, B, dG.data_ptr(), _ptr(goff), G, pref, dK.data_ptr(),
                                                      dO.data_ptr()))
        torch.cuda.synchronize(dev)                     # (the device: the refit runs on the handle's own stream)
        return dK.cpu().numpy().reshape(-1)[:G * NK].reshape(G, NK), dO.cpu().numpy()

    def discover_rows(self, programs, X, target, lengths=None, group_off=None, params=None, return_gram: bool = False,
                      device: bool = False):
        """Rows of sizes 1 .. S chosen from M compiled terms on G groups of recordings (rovmpc_discover_rows; law in
        include/rovmpc.h).  ``programs`` as in ``score_rows``, one per term; X (B, T, F), target (B, T), lengths (B,) or None,
        group_off int32 (G + 1,) or None (all recordings pooled), params a DiscoverParams or None, checked and laid out by
        ``scoring.discover_rows``.  Returns (picks (G, S) int32, coef (G, S, S), loss (G, S + 1), info (G, 3) int64, gram
        (G, (M + 1)(M + 2) / 2) or None).  ``device=True`` goes through rovmpc_discover_rows_device: the same bits."""
        code_off, const_off = [0], [0]
        for code, consts in programs:
            code_off.append(code_off[-1] + len(code)); const_off.append(const_off[-1] + len(consts))
        code = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in programs]), np.int32)
        consts = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float64).reshape(-1) for _, k in programs] + [np.zeros(1)]))
        code_off, const_off = np.asarray(code_off, np.int32), np.asarray(const_off, np.int32)
        M, (B, T, F) = len(programs), X.shape
        G = 1 if group_off is None else len(group_off) - 1
        goff = None if group_off is None else np.ascontiguousarray(group_off, np.int32)
        lens = None if lengths is None else np.ascontiguousarray(lengths, np.int64)
        if params is None:
            params = _lib.DiscoverParams.make()
        S, E = int(params.max_terms), (M + 1) * (M + 2) // 2
        head = (self._h, _ptr(code), _ptr(code_off), _ptr(consts), _ptr(const_off), M)
        if not device:
            picks, coef, loss = np.empty((G, S), np.int32), np.empty((G, S, S)), np.empty((G, S + 1))
            info = np.empty((G, 3), np.int64)
            gram = np.empty((G, E)) if return_gram else None
            self._check(self.lib.rovmpc_discover_rows(*head, _ptr(X), F, _ptr(lens), T, B, _ptr(target), _ptr(goff), G, C.byref(params),
                                                      _ptr(picks), _ptr(coef), _ptr(loss), _ptr(info), _ptr(gram)))
            return picks, coef, loss, info, gram
        import torch
        dev = torch.device("cuda", self.cfg.device)
        dX, dT = torch.tensor(X, device=dev), torch.tensor(target, device=dev)
        dK = torch.empty((G, S), dtype=torch.int32, device=dev)
        dC = torch.empty((G, S, S), dtype=torch.float64, device=dev)
        dL = torch.empty((G, S + 1), dtype=torch.float64, device=dev)
        dI = torch.empty((G, 3), dtype=torch.int64, device=dev)
        dG = torch.empty((G, E), dtype=torch.float64, device=dev) if return_gram else None
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_discover_rows_device(*head, dX.data_ptr(), F, _ptr(lens), T, B, dT.data_ptr(), _ptr(goff), G,
                                                         C.byref(params), dK.data_ptr(), dC.data_ptr(), dL.data_ptr(), dI.data_ptr(),
                                                         None if dG is None else dG.data_ptr()))
        torch.cuda.synchronize(dev)                     # (the device: the discovery runs on the handle's own stream)
        return dK.cpu().numpy(), dC.cpu().numpy(), dL.cpu().numpy(), dI.cpu().numpy(), None if dG is None else dG.cpu().numpy()

    def score_pairs(self, theta_programs, gamma_programs, pairs, X, time, theta, gamma, mean, scale, params, lengths=None,
                    return_pred: bool = False, device: bool = False):
        """Q (theta row, gamma row) pairs rolled ``params.H`` steps on their own predictions from every start row of B
        recordings (rovmpc_score_pairs; law in include/rovmpc.h).  The two fronts as ``programs`` of ``score_rows``; pairs
        int32 (Q, 2); X (B, T, F) scaled rows, time, theta, gamma (B, T), mean and scale (F,), params a HorizonParams, lengths
        (B,) or None, checked and laid out by ``scoring.score_pairs``.  Returns (skill (Q, B, H, 9), pred (Q, B, W, H, 2) or
        None).  ``device=True`` goes through rovmpc_score_pairs_device on torch buffers: the same bits."""
        def front(programs):
            code_off, const_off = [0], [0]
            for code, consts in programs:
                code_off.append(code_off[-1] + len(code)); const_off.append(const_off[-1] + len(consts))
            code = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in programs]), np.int32)
            consts = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float64).reshape(-1) for _, k in programs] + [np.zeros(1)]))
            return code, np.asarray(code_off, np.int32), consts, np.asarray(const_off, np.int32), len(programs)
        ct, cot, kt, kot, Rt = front(theta_programs)
        cg, cog, kg, kog, Rg = front(gamma_programs)
        pairs = np.ascontiguousarray(pairs, np.int32)
        mean, scale = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(scale, np.float64)
        Q, (B, T, F), H = len(pairs), X.shape, int(params.H)
        W = (T - 1 - H) // int(params.stride) + 1 if T - 1 - H >= 0 else 0
        lens = None if lengths is None else np.ascontiguousarray(lengths, np.int64)
        head = (self._h, _ptr(ct), _ptr(cot), _ptr(kt), _ptr(kot), Rt, _ptr(cg), _ptr(cog), _ptr(kg), _ptr(kog), Rg, _ptr(pairs), Q)
        if not device:
            skill = np.empty((Q, B, H, _lib.HORIZON_COLS))
            pred = np.empty((Q, B, W, H, 2)) if return_pred else None
            self._check(self.lib.rovmpc_score_pairs(*head, _ptr(X), F, _ptr(mean), _ptr(scale), _ptr(time), _ptr(lens), T, B, _ptr(theta),
                                                    _ptr(gamma), C.byref(params), _ptr(skill), _ptr(pred) if W else None))
            return skill, pred
        import torch
        dev = torch.device("cuda", self.cfg.device)
        dX, dT, dA, dG = (torch.tensor(x, device=dev) for x in (X, time, theta, gamma))
        dS = torch.empty((Q, B, H, _lib.HORIZON_COLS), dtype=torch.float64, device=dev)
        dP = torch.empty((Q, B, W, H, 2), dtype=torch.float64, device=dev) if return_pred else None
        torch.cuda.synchronize(dev)
        self._check(self.lib.rovmpc_score_pairs_device(*head, dX.data_ptr(), F, _ptr(mean), _ptr(scale), dT.data_ptr(), _ptr(lens), T, B,
                                                       dA.data_ptr(), dG.data_ptr(), C.byref(params), dS.data_ptr(),
                                                       dP.data_ptr() if return_pred and W else None))
        torch.cuda.synchronize(dev)                     # (the device: the scoring runs on the handle's own stream)
        return dS.cpu().numpy(), None if dP is None else dP.cpu().numpy()


_default_engine: Optional[Engine] = None


def default_engine() -> Engine:
    """Small shared handle for the stateless helper mirrors (geometry, predict, replay)."""
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(MPCConfig(N=1, K=1))
    return _default_engine
