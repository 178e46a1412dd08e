"""ctypes binding of librovmpc.so (include/rovmpc.h).  No CPU fallback: if the HIP library
is missing or no GPU is present every compute entry point raises ``RovmpcError``."""
from __future__ import annotations

import ctypes as C
import math
import numbers
import os
from typing import Optional

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "librovmpc.so")

F64, F32 = 0, 1
VT_NONE, VT_COMPOSE, VT_TABLE = 0, 1, 2
PREV_INTERP, PREV_HOLD = 0, 1
RK4, EULER, DOUBLE_EULER, TRAPEZOID = 0, 1, 2, 3
ENU, NED = 0, 1
FEATURES_GEN1, FEATURES_GEN2, FEATURES_GEN3 = 0, 1, 2
STATE_LEN = 16

ERR_NAMES = {0: "OK", -1: "ROVMPC_ERR_INVALID", -2: "ROVMPC_ERR_HIP", -3: "ROVMPC_ERR_NO_MODEL",
             -4: "ROVMPC_ERR_UNSUPPORTED"}


# rovmpc_probe_fn of include/rovmpc.h, in the header's order
PROBE_FN = {name: i for i, name in enumerate((
    "SIN", "SIN_PINNED", "SIN_BOUNDED", "SINCOS", "SINCOS_PINNED", "RCP", "DIV", "DIVQ", "DIVX", "SQRTQ", "SQRT", "MIN_RAW",
    "EXP_INC", "EXP_INC_TINY", "SINH_POS", "SINHC_M1_SMALL", "COSH_M1_SMALL"))}
PROBE_TWO_OPERANDS = ("DIV", "DIVQ", "DIVX", "MIN_RAW")
PROBE_TWO_RESULTS = ("SINCOS", "SINCOS_PINNED")


class RovmpcError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {message}")
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32), ("dtype", C.c_int32), ("N", C.c_int32),
        ("K", C.c_int32), ("n_shape_pts", C.c_int32), ("vt_mode", C.c_int32), ("prev_mode", C.c_int32),
        ("integrator", C.c_int32), ("frame", C.c_int32), ("force_interpreter", C.c_int32),
        ("candidates_per_block", C.c_int32), ("debug_flags", C.c_int32), ("jit_off", C.c_int32),
        ("feature_map", C.c_int32), ("threads_per_block", C.c_int32), ("no_builtin", C.c_int32),
        ("dt", C.c_double), ("v_scale", C.c_double), ("L", C.c_double), ("cable_wet_weight", C.c_double),
        ("c_lo", C.c_double), ("c_hi", C.c_double),
        ("w_theta", C.c_double), ("w_gamma", C.c_double), ("w_u", C.c_double), ("w_T", C.c_double),
        ("w_taut", C.c_double), ("rho_taut", C.c_double), ("w_floor", C.c_double), ("z_floor", C.c_double),
        ("theta_ref", C.c_double), ("gamma_ref", C.c_double), ("U_ref", C.c_double * 3),
    ]


class State(C.Structure):
    _fields_ = [("P0", C.c_double * 3), ("P1", C.c_double * 3), ("V1", C.c_double * 3), ("A1", C.c_double * 3),
                ("theta", C.c_double), ("gamma", C.c_double), ("theta_prev", C.c_double), ("gamma_prev", C.c_double)]


class MPPIParams(C.Structure):
    """Mirror of ``rovmpc_mppi_params``.  ``make`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("n_iter", C.c_int32), ("lambda_", C.c_double), ("std", C.c_double * 3)]

    @classmethod
    def make(cls, n_iter: int = 1, lam: float = 1.0, std=(0.0, 0.0, 0.0)) -> "MPPIParams":
        import math
        if isinstance(n_iter, bool) or int(n_iter) != n_iter or not 1 <= int(n_iter) <= 64:
            raise ValueError(f"n_iter must be an integer in 1..64 (got {n_iter!r})")
        lam = float(lam)
        if not (math.isfinite(lam) and lam > 0):
            raise ValueError(f"lambda must be finite and > 0 (got {lam!r})")
        sd = [float(v) for v in std]
        if len(sd) != 3 or not all(math.isfinite(v) and v >= 0 for v in sd):
            raise ValueError(f"std must be 3 finite values >= 0 (got {std!r})")
        p = cls()
        p.struct_size = C.sizeof(cls)
        p.n_iter = int(n_iter)
        p.lambda_ = lam
        p.std = (C.c_double * 3)(*sd)
        return p


class CEMParams(C.Structure):
    """Mirror of ``rovmpc_cem_params``.  ``make`` checks the values before the library sees them (n_elite <= K is checked by
    the library and by ``rovmpc.CEM``, which know K)."""
    _fields_ = [("struct_size", C.c_int32), ("n_iter", C.c_int32), ("n_elite", C.c_int32), ("reserved", C.c_int32),
                ("alpha", C.c_double), ("std", C.c_double * 3), ("std_min", C.c_double * 3),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3)]

    @classmethod
    def make(cls, n_iter: int = 1, n_elite: int = 1, alpha: float = 0.0, std=(0.0, 0.0, 0.0), std_min=(0.0, 0.0, 0.0),
             lo=(-math.inf,) * 3, hi=(math.inf,) * 3, reserved: int = 0) -> "CEMParams":
        def integer(name, v, lo_, hi_):
            if isinstance(v, bool) or int(v) != v or not lo_ <= int(v) <= hi_:
                raise ValueError(f"{name} must be an integer in {lo_}..{hi_} (got {v!r})")
            return int(v)

        def triple(name, v, ok, what):
            t = [float(x) for x in v]
            if len(t) != 3 or not all(ok(x) for x in t):
                raise ValueError(f"{name} must be 3 values, {what} (got {v!r})")
            return t
        n_iter = integer("n_iter", n_iter, 1, 64)
        n_elite = integer("n_elite", n_elite, 1, 1024)
        if reserved != 0:
            raise ValueError(f"reserved must be 0 (got {reserved!r})")
        alpha = float(alpha)
        if not (math.isfinite(alpha) and 0.0 <= alpha < 1.0):
            raise ValueError(f"alpha must be finite and 0 <= alpha < 1 (got {alpha!r})")
        sd = triple("std", std, lambda x: math.isfinite(x) and x >= 0, "finite and >= 0")
        sm = triple("std_min", std_min, lambda x: math.isfinite(x) and x >= 0, "finite and >= 0")
        lo = triple("lo", lo, lambda x: not math.isnan(x), "not NaN")
        hi = triple("hi", hi, lambda x: not math.isnan(x), "not NaN")
        if not all(a <= b for a, b in zip(lo, hi)):
            raise ValueError(f"lo must be <= hi on every channel (got {lo!r}, {hi!r})")
        p = cls()
        p.struct_size = C.sizeof(cls)
        p.n_iter, p.n_elite, p.reserved, p.alpha = n_iter, n_elite, 0, alpha
        p.std, p.std_min = (C.c_double * 3)(*sd), (C.c_double * 3)(*sm)
        p.lo, p.hi = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
        return p


def noise_correlation(beta):
    """beta of ``rovmpc_set_noise_correlation`` checked before the library sees it: None (white noise), or 3 finite values
    with 0 <= beta < 1.  Returns None or the list of 3 floats."""
    if beta is None:
        return None
    b = [float(v) for v in beta]
    if len(b) != 3 or not all(math.isfinite(v) and 0.0 <= v < 1.0 for v in b):
        raise ValueError(f"beta must be 3 finite values with 0 <= beta < 1 (got {beta!r})")
    return b


def control_box(lo, hi):
    """lo, hi of ``rovmpc_mppi_set_bounds`` checked before the library sees them: both None (unbounded), or 3 values each, not
    NaN, lo <= hi (+-inf allowed).  Returns None or (lo, hi) as lists of 3 floats."""
    if lo is None and hi is None:
        return None
    if lo is None or hi is None:
        raise ValueError(f"lo and hi must both be given or both be None (got {lo!r}, {hi!r})")
    lo_, hi_ = [float(v) for v in lo], [float(v) for v in hi]
    for name, t, v in (("lo", lo_, lo), ("hi", hi_, hi)):
        if len(t) != 3 or any(math.isnan(x) for x in t):
            raise ValueError(f"{name} must be 3 values, not NaN (got {v!r})")
    if not all(a <= b for a, b in zip(lo_, hi_)):
        raise ValueError(f"lo must be <= hi on every channel (got {lo!r}, {hi!r})")
    return lo_, hi_


NAV_MAX_SPHERES = 8
NAV_MAX_ROWS = 1 << 24


class NavCost(C.Structure):
    """Mirror of ``rovmpc_nav_cost``.  ``nav_cost`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("n_spheres", C.c_int32), ("w_pos", C.c_double * 3), ("w_term", C.c_double * 3),
                ("w_du", C.c_double * 3), ("w_sphere", C.c_double), ("spheres", (C.c_double * 4) * NAV_MAX_SPHERES),
                ("origin", C.c_uint64)]


def nav_cost(tracks, w_pos=0.0, w_term=0.0, w_du=0.0, w_sphere=0.0, spheres=(), origin=0):
    """The arguments of ``rovmpc_set_nav_cost`` checked before the library sees them: weights finite and >= 0 (a scalar is
    repeated on the three channels), at most 8 spheres (cx, cy, cz, R) finite with R >= 0, tracks (Tr, 3) or (Bt, Tr, 3)
    finite with Bt, Tr >= 1 and Bt * Tr <= 2^24, origin an integer (taken mod 2^64).  Returns (NavCost, tracks (Bt, Tr, 3)
    float64 C-contiguous)."""
    import numpy as np

    def weight3(name, v):
        a = np.asarray(v, dtype=np.float64)
        if a.shape == ():
            a = np.repeat(a, 3)
        if a.shape != (3,) or not all(math.isfinite(x) and x >= 0 for x in a):
            raise ValueError(f"{name} must be a scalar or 3 values, finite and >= 0 (got {v!r})")
        return [float(x) for x in a]
    wp, wt, wd = weight3("w_pos", w_pos), weight3("w_term", w_term), weight3("w_du", w_du)
    ws = float(w_sphere)
    if not (math.isfinite(ws) and ws >= 0):
        raise ValueError(f"w_sphere must be finite and >= 0 (got {w_sphere!r})")
    sp = np.asarray(spheres, dtype=np.float64)
    if sp.size == 0:
        sp = np.empty((0, 4))
    if sp.shape == (4,):
        sp = sp[None]
    if sp.ndim != 2 or sp.shape[1] != 4:
        raise ValueError(f"spheres must have shape (n, 4): cx, cy, cz, R (got {sp.shape})")
    if len(sp) > NAV_MAX_SPHERES:
        raise ValueError(f"at most {NAV_MAX_SPHERES} spheres (got {len(sp)})")
    if not (np.isfinite(sp).all() and (sp[:, 3] >= 0).all()):
        raise ValueError(f"spheres must be finite with R >= 0 (got {spheres!r})")
    if isinstance(origin, bool) or int(origin) != origin:
        raise ValueError(f"origin must be an integer (got {origin!r})")
    tr = np.asarray(tracks, dtype=np.float64)
    if tr.ndim == 2:
        tr = tr[None]
    if tr.ndim != 3 or tr.shape[2] != 3 or tr.shape[0] < 1 or tr.shape[1] < 1:
        raise ValueError(f"track must have shape (Tr, 3) or (Bt, Tr, 3) with Bt, Tr >= 1 (got {np.shape(tracks)})")
    if tr.shape[0] * tr.shape[1] > NAV_MAX_ROWS:
        raise ValueError(f"track has {tr.shape[0] * tr.shape[1]} rows; at most {NAV_MAX_ROWS}")
    if not np.isfinite(tr).all():
        raise ValueError("track must be finite")
    n = NavCost()
    n.struct_size, n.n_spheres = C.sizeof(NavCost), len(sp)
    n.w_pos, n.w_term, n.w_du, n.w_sphere = (C.c_double * 3)(*wp), (C.c_double * 3)(*wt), (C.c_double * 3)(*wd), ws
    for j, row in enumerate(sp):
        n.spheres[j] = (C.c_double * 4)(*[float(x) for x in row])
    n.origin = int(origin) & 0xFFFFFFFFFFFFFFFF
    return n, np.ascontiguousarray(tr)


TETHER_MAX_SPHERES = 8


class TetherCost(C.Structure):
    """Mirror of ``rovmpc_tether_cost``.  ``tether_cost`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("n_spheres", C.c_int32), ("w", C.c_double), ("margin", C.c_double),
                ("spheres", (C.c_double * 4) * TETHER_MAX_SPHERES)]


def tether_cost(spheres, w, margin=0.0):
    """The arguments of ``rovmpc_set_tether_cost`` checked before the library sees them: 1 to 8 spheres (cx, cy, cz, R) finite
    with R >= 0, w and margin finite and >= 0.  Returns a TetherCost."""
    import numpy as np
    for name, v in (("w", w), ("margin", margin)):
        if isinstance(v, (str, bytes)) or not np.isscalar(v):
            raise TypeError(f"{name} must be a number (got {v!r})")
        if not (math.isfinite(float(v)) and float(v) >= 0):
            raise ValueError(f"{name} must be finite and >= 0 (got {v!r})")
    sp = np.asarray(spheres, dtype=np.float64)
    if sp.shape == (4,):
        sp = sp[None]
    if sp.ndim != 2 or sp.shape[1] != 4:
        raise ValueError(f"spheres must have shape (n, 4): cx, cy, cz, R (got {sp.shape})")
    if not 1 <= len(sp) <= TETHER_MAX_SPHERES:
        raise ValueError(f"1 to {TETHER_MAX_SPHERES} spheres (got {len(sp)})")
    if not (np.isfinite(sp).all() and (sp[:, 3] >= 0).all()):
        raise ValueError(f"spheres must be finite with R >= 0 (got {spheres!r})")
    t = TetherCost()
    t.struct_size, t.n_spheres, t.w, t.margin = C.sizeof(TetherCost), len(sp), float(w), float(margin)
    for j, row in enumerate(sp):
        t.spheres[j] = (C.c_double * 4)(*[float(x) for x in row])
    return t


FIT_MAX_MARKERS = 16
FIT_OUT = 6


class FitParams(C.Structure):
    """Mirror of ``rovmpc_fit_params``.  ``make`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("max_iter", C.c_int32), ("tol", C.c_double)]

    @classmethod
    def make(cls, tol: float = 1e-12, max_iter: int = 40) -> "FitParams":
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) <= 1000:
            raise ValueError(f"max_iter must be an integer in 1..1000 (got {max_iter!r})")
        tol = float(tol)
        if not tol >= 0:
            raise ValueError(f"tol must be >= 0 (got {tol!r})")
        p = cls()
        p.struct_size, p.max_iter, p.tol = C.sizeof(cls), int(max_iter), tol
        return p


CALIB_GROUP_OUT = 8
CALIB_FRAME_OUT = 5


class CalibParams(C.Structure):
    """Mirror of ``rovmpc_calib_params``.  ``make`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("max_iter", C.c_int32), ("free_length", C.c_int32), ("reserved_", C.c_int32),
                ("L0", C.c_double), ("L_lo", C.c_double), ("L_hi", C.c_double), ("tol", C.c_double), ("tol_L", C.c_double)]

    @classmethod
    def make(cls, L0=None, free_length: bool = True, L_lo: float = 0.0, L_hi: float = float("inf"), tol: float = 1e-12,
             tol_L: float = 1e-12, max_iter: int = 60) -> "CalibParams":
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) <= 1000:
            raise ValueError(f"max_iter must be an integer in 1..1000 (got {max_iter!r})")
        tol, tol_L, L_lo, L_hi = float(tol), float(tol_L), float(L_lo), float(L_hi)
        if not tol >= 0 or not tol_L >= 0:
            raise ValueError(f"tol and tol_L must be >= 0 (got {tol!r}, {tol_L!r})")
        if L0 is not None and not (math.isfinite(float(L0)) and float(L0) > 0):
            raise ValueError(f"L0 must be positive and finite (got {L0!r})")
        if not L_lo < L_hi:
            raise ValueError(f"the box (L_lo, L_hi) is empty (got {L_lo!r}, {L_hi!r})")
        p = cls()
        p.struct_size, p.max_iter, p.free_length = C.sizeof(cls), int(max_iter), int(bool(free_length))
        p.L0 = float("nan") if L0 is None else float(L0)
        p.L_lo, p.L_hi, p.tol, p.tol_L = L_lo, L_hi, tol, tol_L
        return p


TRACK_MAX_STARTS = 8
TRACK_OUT = 9
TRACK_DEFAULT_STARTS = ((0.0, 0.0), (0.3, 0.0), (-0.3, 0.0), (0.6, 0.0), (-0.6, 0.0))


class TrackParams(C.Structure):
    """Mirror of ``rovmpc_track_params``.  ``make`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("n_starts", C.c_int32), ("max_iter", C.c_int32), ("reserved_", C.c_int32),
                ("tol", C.c_double), ("rms_max", C.c_double), ("starts", (C.c_double * 2) * TRACK_MAX_STARTS)]

    @classmethod
    def make(cls, starts=None, rms_max: float = float("inf"), tol: float = 1e-12, max_iter: int = 40) -> "TrackParams":
        f = FitParams.make(tol, max_iter)
        starts = [tuple(float(x) for x in s) for s in (TRACK_DEFAULT_STARTS if starts is None else starts)]
        if not 1 <= len(starts) <= TRACK_MAX_STARTS or any(len(s) != 2 for s in starts):
            raise ValueError(f"starts must be 1..{TRACK_MAX_STARTS} pairs (theta, gamma) (got {starts!r})")
        if not all(math.isfinite(x) for s in starts for x in s):
            raise ValueError(f"starts must be finite (got {starts!r})")
        rms_max = float(rms_max)
        if not rms_max > 0:
            raise ValueError(f"rms_max must be > 0 (got {rms_max!r})")
        p = cls()
        p.struct_size, p.n_starts, p.max_iter, p.tol, p.rms_max = C.sizeof(cls), len(starts), f.max_iter, f.tol, rms_max
        for k, s in enumerate(starts):
            p.starts[k][0], p.starts[k][1] = s
        return p


SCORE_COLS = 8
SCORE_TILE = 128
SCORE_NAMES = ("r2", "rmse", "max_abs", "n_finite", "loss", "r2_deriv", "last", "ss_res")
MAX_FEATURES = 32

REFIT_MAX_PARAMS = 8
REFIT_OUT = 6
REFIT_NAMES = ("loss0", "loss", "orth", "iters", "status", "n_params")
REFIT_CONVERGED, REFIT_MAX_ITER, REFIT_STALLED, REFIT_NONFINITE, REFIT_NO_PARAMS = range(5)


class RefitParams(C.Structure):
    """Mirror of ``rovmpc_refit_params``.  ``make`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("max_iter", C.c_int32), ("gtol", C.c_double), ("xtol", C.c_double)]

    @classmethod
    def make(cls, max_iter: int = 50, gtol: float = 1e-10, xtol: float = 1e-12) -> "RefitParams":
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) <= 1000:
            raise ValueError(f"max_iter must be an integer in 1..1000 (got {max_iter!r})")
        gtol, xtol = float(gtol), float(xtol)
        if not gtol >= 0 or not xtol >= 0:
            raise ValueError(f"gtol and xtol must be >= 0 (got {gtol!r}, {xtol!r})")
        p = cls()
        p.struct_size, p.max_iter, p.gtol, p.xtol = C.sizeof(cls), int(max_iter), gtol, xtol
        return p


DISCOVER_MAX_TERMS = 64
DISCOVER_MAX_SIZE = 8
DISCOVER_CHUNK = 1024
DISCOVER_FULL, DISCOVER_MIN_GAIN, DISCOVER_EXHAUSTED, DISCOVER_NONFINITE = range(4)


class DiscoverParams(C.Structure):
    """Mirror of ``rovmpc_discover_params``.  ``make`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("max_terms", C.c_int32), ("dep_tol", C.c_double), ("min_gain", C.c_double)]

    @classmethod
    def make(cls, max_terms: int = 8, dep_tol: float = 1e-10, min_gain: float = 1e-12) -> "DiscoverParams":
        if isinstance(max_terms, bool) or int(max_terms) != max_terms or not 1 <= int(max_terms) <= DISCOVER_MAX_SIZE:
            raise ValueError(f"max_terms must be an integer in 1..{DISCOVER_MAX_SIZE} (got {max_terms!r})")
        dep_tol, min_gain = float(dep_tol), float(min_gain)
        if not dep_tol >= 0 or not min_gain >= 0:
            raise ValueError(f"dep_tol and min_gain must be >= 0 (got {dep_tol!r}, {min_gain!r})")
        p = cls()
        p.struct_size, p.max_terms, p.dep_tol, p.min_gain = C.sizeof(cls), int(max_terms), dep_tol, min_gain
        return p


HORIZON_COLS = 9
HORIZON_TILE = 128
HORIZON_NAMES = ("rmse_theta", "rmse_gamma", "max_abs_theta", "max_abs_gamma", "n_ok", "ss_theta", "ss_gamma", "ss_hold_theta",
                 "ss_hold_gamma")
HORIZON_SLOTS = ("theta", "gamma", "theta_prev", "gamma_prev", "cos_theta", "sin_gamma")
# the reference's two first-order feature maps: which slots of a row the pair's own state is written to (-1: none)
FEATURE_MAPS = {"gen1": (14, 15, 16, 17, -1, -1), "gen2": (12, 13, -1, -1, 14, 15)}


class HorizonParams(C.Structure):
    """Mirror of ``rovmpc_horizon_params``.  ``make`` checks the values before the library sees them."""
    _fields_ = [("struct_size", C.c_int32), ("integrator", C.c_int32), ("prev_mode", C.c_int32), ("H", C.c_int32), ("stride", C.c_int32)] + \
               [("slot_" + n, C.c_int32) for n in HORIZON_SLOTS]

    @classmethod
    def make(cls, H: int = 20, stride: int = 1, integrator: int = RK4, prev_mode: int = PREV_INTERP, slots=FEATURE_MAPS["gen1"],
             F: Optional[int] = None) -> "HorizonParams":
        for name, v in (("horizon", H), ("stride", stride)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= int(v) < 2 ** 31:
                raise ValueError(f"{name} must be an integer >= 1 (got {v!r})")
        if integrator not in (RK4, EULER):
            raise ValueError(f"integrator must be RK4 or EULER (got {integrator!r}; the second-order maps are not provided)")
        if prev_mode not in (PREV_INTERP, PREV_HOLD):
            raise ValueError(f"prev_mode must be PREV_INTERP or PREV_HOLD (got {prev_mode!r})")
        slots = tuple(slots)
        if len(slots) != len(HORIZON_SLOTS) or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in slots):
            raise ValueError(f"slots must be {len(HORIZON_SLOTS)} integers {HORIZON_SLOTS} (got {slots!r})")
        slots = tuple(int(v) for v in slots)
        if slots[0] == -1 or slots[1] == -1:
            raise ValueError("the theta and gamma slots are required")
        used = [v for v in slots if v != -1]
        if any(v < 0 or (F is not None and v >= F) for v in used):
            raise ValueError(f"a named slot is outside 0..{'F - 1' if F is None else F - 1} (got {slots!r})")
        if len(set(used)) != len(used):
            raise ValueError(f"two names on one slot (got {slots!r})")
        p = cls()
        p.struct_size, p.integrator, p.prev_mode, p.H, p.stride = C.sizeof(cls), int(integrator), int(prev_mode), int(H), int(stride)
        for n, v in zip(HORIZON_SLOTS, slots):
            setattr(p, "slot_" + n, v)
        return p

    def slots(self):
        return tuple(getattr(self, "slot_" + n) for n in HORIZON_SLOTS)


_P = C.c_void_p
_SIGNATURES = {
    "rovmpc_version": (C.c_char_p, []),
    "rovmpc_default_config": (None, [C.POINTER(Config)]),
    "rovmpc_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "rovmpc_destroy": (None, [_P]),
    "rovmpc_last_error": (C.c_char_p, [_P]),
    "rovmpc_set_model": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32]),
    "rovmpc_set_rotation_table": (C.c_int, [_P, _P]),
    "rovmpc_model_path": (C.c_int32, [_P]),
    "rovmpc_model_structure": (C.c_int32, [_P]),
    "rovmpc_step": (C.c_int, [_P, C.POINTER(State), _P, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "rovmpc_rollout_costs": (C.c_int, [_P, C.POINTER(State), _P, _P, _P]),
    "rovmpc_mppi_reset": (C.c_int, [_P, _P]),
    "rovmpc_mppi_step": (C.c_int, [_P, C.POINTER(State), C.c_uint64, C.c_uint64, C.POINTER(MPPIParams), _P, _P, _P]),
    "rovmpc_mppi_last": (C.c_int, [_P, _P, _P]),
    "rovmpc_mppi_update_device": (C.c_int, [_P, _P, _P, C.c_double, _P, _P, _P, _P]),
    "rovmpc_cem_reset": (C.c_int, [_P, _P]),
    "rovmpc_cem_step": (C.c_int, [_P, C.POINTER(State), C.c_uint64, C.c_uint64, C.POINTER(CEMParams), _P, _P, _P, _P, _P]),
    "rovmpc_cem_last": (C.c_int, [_P, _P, _P]),
    "rovmpc_cem_update_device": (C.c_int, [_P, _P, _P, C.POINTER(CEMParams), _P, _P, _P, _P, _P, _P, _P]),
    "rovmpc_mppi_reset_batch": (C.c_int, [_P, C.c_int32, _P]),
    "rovmpc_mppi_step_batch": (C.c_int, [_P, C.c_int32, _P, _P, C.c_uint64, C.POINTER(MPPIParams), _P, _P, _P]),
    "rovmpc_mppi_last_batch": (C.c_int, [_P, _P, _P]),
    "rovmpc_cem_reset_batch": (C.c_int, [_P, C.c_int32, _P]),
    "rovmpc_cem_step_batch": (C.c_int, [_P, C.c_int32, _P, _P, C.c_uint64, C.POINTER(CEMParams), _P, _P, _P, _P, _P]),
    "rovmpc_cem_last_batch": (C.c_int, [_P, _P, _P]),
    "rovmpc_set_noise_correlation": (C.c_int, [_P, _P]),
    "rovmpc_mppi_set_bounds": (C.c_int, [_P, _P, _P]),
    "rovmpc_set_nav_cost": (C.c_int, [_P, C.POINTER(NavCost), _P, C.c_int32, C.c_int64]),
    "rovmpc_nav_cost_device": (C.c_int, [_P, _P, _P, C.c_uint64, _P, _P, _P]),
    "rovmpc_set_tether_cost": (C.c_int, [_P, C.POINTER(TetherCost)]),
    "rovmpc_tether_cost_device": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "rovmpc_default_fit_params": (None, [C.POINTER(FitParams)]),
    "rovmpc_fit_theta_gamma": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, _P, C.POINTER(FitParams), _P]),
    "rovmpc_fit_theta_gamma_device": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, _P, C.POINTER(FitParams), _P]),
    "rovmpc_default_calib_params": (None, [C.POINTER(CalibParams)]),
    "rovmpc_calibrate_cable": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(CalibParams), _P, _P]),
    "rovmpc_calibrate_cable_device": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(CalibParams), _P, _P]),
    "rovmpc_cable_markers": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P]),
    "rovmpc_default_track_params": (None, [C.POINTER(TrackParams)]),
    "rovmpc_track_markers": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, C.POINTER(TrackParams), _P]),
    "rovmpc_track_markers_device": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, C.POINTER(TrackParams), _P, _P]),
    "rovmpc_mppi_row_len": (C.c_int32, [_P]),
    "rovmpc_cem_row_len": (C.c_int32, [_P, C.c_int32]),
    "rovmpc_mppi_closed_loop_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(MPPIParams), _P]),
    "rovmpc_cem_closed_loop_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(CEMParams), _P]),
    "rovmpc_mppi_closed_loop_batch_device": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int32, _P, C.c_uint64, C.POINTER(MPPIParams), _P]),
    "rovmpc_cem_closed_loop_batch_device": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int32, _P, C.c_uint64, C.POINTER(CEMParams), _P]),
    "rovmpc_mpc_step_sampled": (C.c_int, [_P, C.POINTER(State), C.c_uint64, C.c_uint64, _P, _P, C.c_int32, _P]),
    "rovmpc_sampled_candidates": (C.c_int, [_P, _P]),
    "rovmpc_sample_candidates_device": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    "rovmpc_result_len": (C.c_int32, [_P]),
    "rovmpc_step_device": (C.c_int, [_P, _P, _P, _P, _P]),
    "rovmpc_step_device_sharded": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    "rovmpc_select_device": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "rovmpc_comm_unique_id": (C.c_int, [_P]),
    "rovmpc_comm_init": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "rovmpc_step_device_allreduce": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P]),
    "rovmpc_comm_join": (C.c_int, [_P, _P]),
    "rovmpc_comm_sync": (C.c_int, [_P, _P]),
    "rovmpc_comm_placement": (C.c_char_p, [_P]),
    "rovmpc_comm_abort": (C.c_int, [_P]),
    "rovmpc_step_batch_device": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "rovmpc_batch_costs_device": (C.c_int, [_P, C.POINTER(_P)]),
    "rovmpc_set_option": (C.c_int, [_P, C.c_char_p, C.c_double]),
    "rovmpc_device_status": (C.c_int, [_P]),
    "rovmpc_comm_destroy": (C.c_int, [_P]),
    "rovmpc_closed_loop_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P]),
    "rovmpc_closed_loop_pipelined_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "rovmpc_closed_loop_form": (C.c_int32, [_P]),
    "rovmpc_timing_enable": (C.c_int, [_P, C.c_int32]),
    "rovmpc_timing_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "rovmpc_math_probe": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P, _P]),
    "rovmpc_predict": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    "rovmpc_eval_expression": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int64, _P]),
    "rovmpc_lagrangian_rollout": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P]),
    "rovmpc_replay": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, C.c_double, C.c_int32, _P, _P]),
    "rovmpc_score_rows": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int32,
                                    _P, _P, _P]),
    "rovmpc_score_rows_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P, _P,
                                           C.c_int32, _P, _P, _P]),
    "rovmpc_default_refit_params": (None, [C.POINTER(RefitParams)]),
    "rovmpc_refit_rows": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, C.c_int32,
                                    C.POINTER(RefitParams), _P, _P]),
    "rovmpc_refit_rows_device": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P,
                                           C.c_int32, C.POINTER(RefitParams), _P, _P]),
    "rovmpc_default_discover_params": (None, [C.POINTER(DiscoverParams)]),
    "rovmpc_discover_rows": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, C.c_int32,
                                       C.POINTER(DiscoverParams), _P, _P, _P, _P, _P]),
    "rovmpc_discover_rows_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, C.c_int32,
                                              C.POINTER(DiscoverParams), _P, _P, _P, _P, _P]),
    "rovmpc_default_horizon_params": (None, [C.POINTER(HorizonParams)]),
    "rovmpc_score_pairs": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P,
                                     C.c_int64, C.c_int64, _P, _P, C.POINTER(HorizonParams), _P, _P]),
    "rovmpc_score_pairs_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P,
                                            _P, C.c_int64, C.c_int64, _P, _P, C.POINTER(HorizonParams), _P, _P]),
    "rovmpc_solve_catenary": (C.c_int, [_P, _P, _P, C.c_double, C.c_int64, _P, _P]),
    "rovmpc_rodrigues": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P]),
    "rovmpc_catenary_points": (C.c_int, [_P, _P, _P, C.c_double, C.c_int64, C.c_int32, _P, _P, _P]),
    "rovmpc_compute_catenary_3d": (C.c_int, [_P, _P, _P, C.c_double, C.c_int64, C.c_int32, _P, _P]),
    "rovmpc_transform_catenary": (C.c_int, [_P, _P, _P, _P, _P, C.c_double, C.c_int64, C.c_int32, _P, _P, _P]),
    "rovmpc_velocity_transform": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "rovmpc_extract_features": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P]),
    "rovmpc_gaussian_filter1d": (C.c_int, [_P, _P, C.c_int64, C.c_double, C.c_double, _P]),
    "rovmpc_features_dd": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    "rovmpc_kabsch_velocity_transform": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
}

_lib: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen librovmpc.so and bind every symbol of include/rovmpc.h (loud failure if absent)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ROVMPC_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise RovmpcError(-2, f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64 (same SONAME as the system
    # ROCm).  Two HSA runtimes in one process cannot both own the GPU, so when torch is
    # present it is imported first and librovmpc binds to the runtime torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
        except AttributeError:
            if path is None and os.environ.get("ROVMPC_LIB_OLD_ABI") == "1":
                continue                 # A/B runs against an older build (tools/ab_bench.sh): entry points it lacks stay unbound
            raise
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def exported_symbols():
    return list(_SIGNATURES)


def check(lib, handle, rc: int):
    if rc != 0:
        msg = lib.rovmpc_last_error(handle)
        raise RovmpcError(rc, msg.decode() if msg else "")
