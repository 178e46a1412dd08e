"""Score equation rows on recordings and choose the rows to load (rovmpc_score_rows; law in include/rovmpc.h).

What the reference's evaluation scripts do one row at a time -- integrate the row along a held-out recording and print
``r2_score(truth, est)`` (dd_test_cluster.py:212-247 over both Pareto fronts; simulate_rk4_theta_gamma.py:84-85,
test_cluster.py:145-146, model_test.py:34-35, simulate_theta_gamma.py:108-109 for one row; simply.py:85,98 for the derivative
itself) -- as ONE launch for R rows on B recordings, the scores reduced on the device.

    s = score_rows(rows, X, time, truth, integrator="rk4")     # s.r2, s.rmse, ... each (R, B)
    order = s.rank("r2")                                        # row indices, best first
    model, s_theta, s_gamma = select_model(theta_rows, gamma_rows, X_raw, time, theta, gamma, mean, scale)
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .expr import compile_expression
from .model import DynamicsModel

INTEGRATORS = {"rk4": _lib.RK4, "euler": _lib.EULER, "double_euler": _lib.DOUBLE_EULER, "trapezoid": _lib.TRAPEZOID}
# metric -> whether larger is better
METRICS = {"r2": True, "r2_deriv": True, "n_finite": True, "rmse": False, "max_abs": False, "loss": False, "ss_res": False}
REDUCERS = ("mean", "median", "min", "max")


@dataclass
class RowScores:
    """The eight columns of rovmpc_score_rows, each (R, B); ``est`` / ``pred`` (R, B, T) where they were asked for."""
    r2: np.ndarray
    rmse: np.ndarray
    max_abs: np.ndarray
    n_finite: np.ndarray
    loss: np.ndarray
    r2_deriv: np.ndarray
    last: np.ndarray
    ss_res: np.ndarray
    expressions: Sequence[str] = ()
    est: Optional[np.ndarray] = None
    pred: Optional[np.ndarray] = None

    @classmethod
    def from_table(cls, table, expressions=(), est=None, pred=None) -> "RowScores":
        table = np.asarray(table, dtype=np.float64)
        if table.ndim != 3 or table.shape[2] != _lib.SCORE_COLS:
            raise ValueError(f"scores must be (R, B, {_lib.SCORE_COLS}) (got {table.shape})")
        cols = [np.ascontiguousarray(table[..., k]) for k in range(_lib.SCORE_COLS)]
        cols[3] = cols[3].astype(np.int64)
        return cls(*cols, expressions=tuple(expressions), est=est, pred=pred)

    def table(self) -> np.ndarray:
        return np.stack([np.asarray(getattr(self, n), dtype=np.float64) for n in _lib.SCORE_NAMES], axis=-1)

    def rank(self, metric: str = "r2", reduce: str = "mean") -> np.ndarray:
        """Row indices, best first: the metric reduced over the recordings (a NaN on any recording makes the row's value NaN),
        NaN rows last, ties to the lower index."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {sorted(METRICS)} (got {metric!r})")
        if reduce not in REDUCERS:
            raise ValueError(f"reduce must be one of {REDUCERS} (got {reduce!r})")
        v = np.asarray(getattr(self, metric), dtype=np.float64)
        with np.errstate(all="ignore"):
            v = getattr(np, reduce)(v, axis=1)
        key = -v if METRICS[metric] else v
        key = np.where(np.isnan(key), np.inf, key)                      # NaN last; +inf (the worst finite-side value) before NaN
        nan = np.isnan(v)
        return np.lexsort((np.arange(len(v)), key, nan)).astype(np.int64)

    def best(self, metric: str = "r2", reduce: str = "mean") -> int:
        return int(self.rank(metric, reduce)[0])


def row_text(row) -> str:
    """An expression string, or a row dict of ``read_equation_csv`` (its ``sympy_format``, else its ``equation``)."""
    if isinstance(row, str):
        return row
    if isinstance(row, dict):
        text = row.get("sympy_format") or row.get("equation")
        if isinstance(text, str) and text:
            return text
    raise ValueError(f"a row must be an expression string or a dict with 'sympy_format' / 'equation' (got {row!r})")


def _recordings(X, time, truth, target, lengths, y0):
    """Shapes checked, everything (B, ...) float64 C-contiguous; ``single``: X came as (T, F)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    single = X.ndim == 2
    if single:
        X = X[None]
    if X.ndim != 3:
        raise ValueError(f"X must be (T, F) or (B, T, F) (got {X.shape})")
    B, T, F = X.shape
    if B < 1 or T < 1:
        raise ValueError(f"X needs at least one recording and one time row (got {X.shape})")
    if not 1 <= F <= _lib.MAX_FEATURES:
        raise ValueError(f"1 to {_lib.MAX_FEATURES} features (got {F})")

    def series(name, v):
        a = np.ascontiguousarray(v, dtype=np.float64)
        if single and a.ndim == 1:
            a = a[None]
        if a.shape != (B, T):
            raise ValueError(f"{name} must be {'(T,) or ' if single else ''}(B, T) = {(B, T)} (got {np.shape(v)})")
        return a
    time, truth = series("time", time), series("truth", truth)
    target = None if target is None else series("target", target)
    if lengths is not None:
        lengths = np.asarray(lengths)
        if lengths.shape != (B,) or not np.issubdtype(lengths.dtype, np.integer) or (lengths < 1).any() or (lengths > T).any():
            raise ValueError(f"lengths must be {B} integers in 1..{T} (got {lengths!r})")
        lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    if y0 is not None:
        y0 = np.ascontiguousarray(np.broadcast_to(np.asarray(y0, dtype=np.float64), (B,)) if np.ndim(y0) == 0 else y0, dtype=np.float64)
        if y0.shape != (B,):
            raise ValueError(f"y0 must be a scalar or (B,) = ({B},) (got {y0.shape})")
    return X, time, truth, target, lengths, y0, single


def score_rows(rows, X, time, truth, integrator="rk4", target=None, lengths=None, y0=None, variable_names=None,
               return_est: bool = False, return_pred: bool = False, engine=None, device: bool = False) -> RowScores:
    """Score every row of ``rows`` (expression strings or ``read_equation_csv`` dicts) against ``truth`` on the recordings
    X (T, F) or (B, T, F) of already-scaled feature rows, time and truth (T,) or (B, T).  ``integrator``: "rk4", "euler",
    "double_euler", "trapezoid" (or the library's constants); ``target``: the derivative series the rows were fitted to (for
    ``loss`` and ``r2_deriv``); ``lengths``: the rows of each recording that count; ``y0``: the start, truth[:, 0] if None.
    One launch; no model needs to be loaded."""
    if isinstance(integrator, str):
        if integrator not in INTEGRATORS:
            raise ValueError(f"integrator must be one of {sorted(INTEGRATORS)} (got {integrator!r})")
        integrator = INTEGRATORS[integrator]
    elif integrator not in INTEGRATORS.values():
        raise ValueError(f"unknown integrator {integrator!r}")
    if isinstance(rows, (str, dict)):
        raise ValueError("rows must be a sequence of rows, not a single row")
    texts = [row_text(r) for r in rows]
    if not texts:
        raise ValueError("rows is empty")
    X, time, truth, target, lengths, y0, _ = _recordings(X, time, truth, target, lengths, y0)
    programs = []
    for text in texts:
        consts: list = []
        prog = compile_expression(text, consts, X.shape[2], variable_names)
        programs.append((prog.code, consts))
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    table, est, pred = engine.score_rows(programs, X, time, truth, integrator, target, lengths, y0, return_est, return_pred, device)
    return RowScores.from_table(table, texts, est, pred)


def select_model(theta_rows, gamma_rows, X_raw, time, theta, gamma, mean, scale, integrator="rk4", metric: str = "r2",
                 reduce: str = "mean", lengths=None, variable_names=None, engine=None):
    """Score both Pareto fronts on the recordings and return (the DynamicsModel of the two best rows, theta scores, gamma
    scores).  ``X_raw`` (T, F) or (B, T, F) are unscaled feature rows; they are scaled as the scaler does, (X - mean) / scale,
    before the rows read them.  ``theta`` / ``gamma``: the measured series the replays are held against."""
    mean = np.asarray(mean, dtype=np.float64); scale = np.asarray(scale, dtype=np.float64)
    X_raw = np.asarray(X_raw, dtype=np.float64)
    if mean.ndim != 1 or mean.shape != scale.shape or X_raw.ndim not in (2, 3) or X_raw.shape[-1] != mean.shape[0]:
        raise ValueError(f"mean and scale must be (F,) with F = X_raw.shape[-1] (got {mean.shape}, {scale.shape}, {X_raw.shape})")
    Xs = (X_raw - mean) / scale
    kw = dict(integrator=integrator, lengths=lengths, variable_names=variable_names, engine=engine)
    s_theta = score_rows(theta_rows, Xs, time, theta, **kw)
    s_gamma = score_rows(gamma_rows, Xs, time, gamma, **kw)
    model = DynamicsModel(mean, scale, s_theta.expressions[s_theta.best(metric, reduce)],
                          s_gamma.expressions[s_gamma.best(metric, reduce)], variable_names=variable_names)
    return model, s_theta, s_gamma
