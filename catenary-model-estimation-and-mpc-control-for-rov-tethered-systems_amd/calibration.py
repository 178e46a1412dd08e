"""The cable length from marker recordings, and the forward model with markers placed by arc length (law: include/rovmpc.h
above rovmpc_calibrate_cable).  The arithmetic is the library's; this module shapes the arguments and names the columns."""
from __future__ import annotations

import dataclasses
import enum
from dataclasses import dataclass

import numpy as np

from .engine import CableTrack, default_engine


class CalibStatus(enum.IntEnum):
    """Status of a group (and of its active frames), and the class of a frame that was left out: ``rovmpc_fit_status``
    and the two values rovmpc_calibrate_cable adds (include/rovmpc.h)."""
    CONVERGED = 0
    MAX_ITER = 1
    DEGENERATE = 2
    CHORD = 3
    TOO_FEW = 4
    NONFINITE = 5
    STALLED = 6
    NO_FRAMES = 7


@dataclass(frozen=True)
class CableCalibration:
    """Columns of ``rovmpc_calibrate_cable``'s outputs.  Per group, arrays (G,) (scalars when ``groups="pooled"`` pooled one
    recording): L, sigma_L (its standard error from the residuals, NaN without degrees of freedom or with a fixed length),
    rms, rms0 (metres, at the estimate and at the start), iters (trial steps), status (``CalibStatus``), n_active (frames
    that took part), n_markers (their valid markers).  Per frame, arrays of the shape of the recording(s): theta, gamma,
    frame_rms, frame_rms0, frame_status (an active frame's is its group's; a frame left out keeps its class).
    ``group_off`` (G + 1,): the groups as runs of the flattened frames."""
    L: np.ndarray
    sigma_L: np.ndarray
    rms: np.ndarray
    rms0: np.ndarray
    iters: np.ndarray
    status: np.ndarray
    n_active: np.ndarray
    n_markers: np.ndarray
    theta: np.ndarray
    gamma: np.ndarray
    frame_rms: np.ndarray
    frame_rms0: np.ndarray
    frame_status: np.ndarray
    group_off: np.ndarray

    def config(self, cfg):
        """``cfg`` with its L replaced by the calibrated length.  ValueError unless there is exactly one group and it is
        CONVERGED."""
        if np.size(self.status) != 1:
            raise ValueError(f"config() needs exactly one group (got {np.size(self.status)})")
        status = CalibStatus(int(np.reshape(self.status, -1)[0]))
        if status is not CalibStatus.CONVERGED:
            raise ValueError(f"the calibration did not converge: status {status.name} after {int(np.reshape(self.iters, -1)[0])} trial steps")
        return dataclasses.replace(cfg, L=float(np.reshape(self.L, -1)[0]))


def _group_offsets(groups, B: int, T: int) -> np.ndarray:
    F = B * T
    if isinstance(groups, str):
        if groups == "pooled":                          # one group per recording
            return np.arange(B + 1, dtype=np.int64) * T
        if groups == "each":                            # one group per frame
            return np.arange(F + 1, dtype=np.int64)
        raise ValueError(f'groups must be "pooled", "each" or offsets (got {groups!r})')
    off = np.asarray(groups)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("groups as offsets must be a 1-d integer array of G + 1 entries")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != F or (np.diff(off) < 0).any():
        raise ValueError(f"group offsets must run non-decreasing from 0 to the number of frames {F} (got {off.tolist()})")
    return off


def calibrate_cable(P0, P1, markers, guess=None, arc=None, L0=None, free_length: bool = True, groups="pooled", L_lo: float = 0.0,
                    L_hi: float = float("inf"), tol: float = 1e-12, tol_L: float = 1e-12, max_iter: int = 60, engine=None,
                    device: bool = False) -> CableCalibration:
    """The cable length from a recording of its markers (rovmpc_calibrate_cable): ``markers`` (T, M, 3) or (B, T, M, 3), a NaN
    row = a missing marker; P0, P1 broadcastable to (T, 3) / (B, T, 3); ``guess`` (..., 2) start angles or a ``CableTrack``
    (its angles), (0, 0) if None; ``arc`` (M,): the markers' fractions of the cable's length from 0 to 1 (None: the index
    rule of ``fit_theta_gamma``); ``L0``: the start (None: the engine's L); ``free_length=False`` keeps L at L0 and fits the
    angles alone; ``groups``: "pooled" (one L per recording), "each" (one per frame) or offsets (G + 1,) into the flattened
    frames; (L_lo, L_hi): the box L must stay in.  Returns a ``CableCalibration``.  ``engine``: the one whose bracket and
    frame hold (default: the shared helper engine)."""
    Y = np.ascontiguousarray(markers, np.float64)
    single = Y.ndim == 3
    if single:
        Y = Y[None]
    if Y.ndim != 4 or Y.shape[3] != 3:
        raise ValueError(f"markers must be (T, M, 3) or (B, T, M, 3), got {np.shape(markers)}")
    B, T, M = Y.shape[:3]
    if not 3 <= M <= 16:
        raise ValueError(f"3 to 16 markers per frame (got {M})")
    off = _group_offsets(groups, B, T)
    c = lambda x, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), shape))
    P0, P1 = c(P0, (B, T, 3)), c(P1, (B, T, 3))
    if isinstance(guess, CableTrack):
        guess = np.stack([guess.theta, guess.gamma], axis=-1)
    G0 = None if guess is None else c(guess, (B, T, 2)).reshape(B * T, 2)
    if arc is not None:
        arc = np.ascontiguousarray(arc, np.float64)
        if arc.shape != (M,) or not np.isfinite(arc).all() or arc[0] != 0.0 or arc[-1] != 1.0 or not (np.diff(arc) > 0).all():
            raise ValueError(f"arc must be ({M},), finite and strictly increasing from 0 to 1")
    eng = engine or default_engine()
    og, of = eng.calibrate_cable(P0.reshape(B * T, 3), P1.reshape(B * T, 3), Y.reshape(B * T, M, 3), off.astype(np.int32), guess=G0,
                                 arc=arc, L0=L0, free_length=free_length, L_lo=L_lo, L_hi=L_hi, tol=tol, tol_L=tol_L, max_iter=max_iter,
                                 device=device)
    og, of = np.asarray(og), np.asarray(of)
    scalar = single and isinstance(groups, str) and groups == "pooled"
    gcol = lambda k, t=None: (lambda v: v[0] if scalar else v)(og[:, k] if t is None else og[:, k].astype(t))
    shape = (T,) if single else (B, T)
    fcol = lambda k, t=None: np.ascontiguousarray((of[:, k] if t is None else of[:, k].astype(t)).reshape(shape))
    return CableCalibration(L=gcol(0), sigma_L=gcol(3), rms=gcol(1), rms0=gcol(2), iters=gcol(4, np.int64), status=gcol(5, np.int64),
                            n_active=gcol(6, np.int64), n_markers=gcol(7, np.int64), theta=fcol(0), gamma=fcol(1), frame_rms=fcol(2),
                            frame_rms0=fcol(3), frame_status=fcol(4, np.int64), group_off=off)


def cable_markers(P0, P1, theta, gamma, L=None, arc=None, M: int = 16, engine=None) -> np.ndarray:
    """The markers of the cable between P0 and P1 at (theta, gamma) and length L (rovmpc_cable_markers): the forward model of
    ``calibrate_cable``, for synthesis and plots.  See ``Engine.cable_markers``."""
    return (engine or default_engine()).cable_markers(P0, P1, theta, gamma, L=L, arc=arc, M=M)
