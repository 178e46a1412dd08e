"""Score equation rows on recordings and choose the rows to load (rovmpc_score_rows; law in include/rovmpc.h).

What the reference's evaluation scripts do one row at a time -- integrate the row along a held-out recording and print
``r2_score(truth, est)`` (dd_test_cluster.py:212-247 over both Pareto fronts; simulate_rk4_theta_gamma.py:84-85,
test_cluster.py:145-146, model_test.py:34-35, simulate_theta_gamma.py:108-109 for one row; simply.py:85,98 for the derivative
itself) -- as ONE launch for R rows on B recordings, the scores reduced on the device.

    s = score_rows(rows, X, time, truth, integrator="rk4")     # s.r2, s.rmse, ... each (R, B)
    order = s.rank("r2")                                        # row indices, best first
    model, s_theta, s_gamma = select_model(theta_rows, gamma_rows, X_raw, time, theta, gamma, mean, scale)

The rows carry the constants PySR found on the reference's cable.  ``refit_rows`` tunes them to the caller's recordings
(rovmpc_refit_rows: what the reference's trainers do for every candidate row, simply.py:65-98, for R given structures in one
launch), and ``select_model(..., refit=True)`` scores and loads the refitted rows.

    fit = refit_rows(rows, X, target)                           # fit.expressions[r][0], fit.loss, fit.status, ... (R, G)

Those scores are open loop: a row is integrated along measured feature rows and never reads its own prediction.  ``score_pairs``
rolls a theta row and a gamma row together on their own predictions, as the controller does, from every start row of a
recording for ``horizon`` steps (rovmpc_score_pairs), and ``select_model(..., horizon=H)`` picks the pair to load by that.

    sk = score_pairs(theta_rows, gamma_rows, X, time, theta, gamma, mean, scale, horizon=20)   # sk.skill_theta, ... (Q, B, H)
    it, ig = sk.pairs[sk.best()]
"""
from __future__ import annotations

import enum
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .expr import OP, compile_expression, rewrite_constants
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


def _recordings(X, time, truth, target, lengths, y0, names=("time", "truth")):
    """Shapes checked, everything (B, ...) float64 C-contiguous; ``single``: X came as (T, F).  ``names``: what the two
    required series are called in the messages."""
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
    time, truth = series(names[0], time), series(names[1], truth)
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


class RefitStatus(enum.IntEnum):
    """``rovmpc_refit_status``: how a fit of ``refit_rows`` ended."""
    CONVERGED = _lib.REFIT_CONVERGED
    MAX_ITER = _lib.REFIT_MAX_ITER
    STALLED = _lib.REFIT_STALLED
    NONFINITE = _lib.REFIT_NONFINITE
    NO_PARAMS = _lib.REFIT_NO_PARAMS


@dataclass
class RowRefit:
    """What rovmpc_refit_rows returns for R rows on G groups.  ``consts[r]``: (G, P_r), all constants of row r (fitted and
    frozen) per group; ``expressions[r][g]``: the row's text with them written in; the six columns each (R, G)."""
    consts: list
    expressions: list
    loss0: np.ndarray
    loss: np.ndarray
    orth: np.ndarray
    iters: np.ndarray
    status: np.ndarray
    n_params: np.ndarray


def exponent_roles(code, n_consts: int):
    """Per constant of a compiled row: (occurrences that reach the exponent operand of a POW, all occurrences).  The stack
    simulation of the library's validation, with the set of PUSH_C occurrences behind every slot."""
    stack, in_exp, seen = [], set(), {}
    for pc, ins in enumerate(code):
        op, arg = ins & 0xFF, ins >> 8
        if op == OP["PUSH_C"]:
            stack.append({pc}); seen.setdefault(arg, set()).add(pc)
        elif op == OP["PUSH_F"]:
            stack.append(set())
        elif op in (OP["ADD"], OP["SUB"], OP["MUL"], OP["DIV"], OP["POW"]):
            b = stack.pop()
            if op == OP["POW"]:
                in_exp |= b
            stack[-1] = stack[-1] | b
    return [(len(seen.get(k, set()) & in_exp), len(seen.get(k, ()))) for k in range(n_consts)]


def default_free(code, n_consts: int, text: str = "") -> np.ndarray:
    """The free mask ``refit_rows`` uses when none is given: every constant but those that occur only as POW exponents."""
    free = np.ones(n_consts, dtype=np.uint8)
    for k, (n_exp, n_all) in enumerate(exponent_roles(code, n_consts)):
        if n_exp and n_exp < n_all:
            raise ValueError(f"constant {k} of {text!r} is shared between a POW exponent and another place: give `free`")
        if n_exp:
            free[k] = 0
    return free


def _group_offsets(groups, B: int):
    """``groups`` of ``refit_rows`` / ``discover_rows`` as the library's group_off: None for "pooled", else int32 offsets."""
    if isinstance(groups, str):
        if groups not in ("pooled", "each"):
            raise ValueError(f"groups must be 'pooled', 'each' or an offsets array (got {groups!r})")
        return None if groups == "pooled" else np.arange(B + 1, dtype=np.int32)
    group_off = np.asarray(groups)
    if group_off.ndim != 1 or len(group_off) < 2 or not np.issubdtype(group_off.dtype, np.integer) or group_off[0] != 0 or \
            group_off[-1] != B or (np.diff(group_off) <= 0).any():
        raise ValueError(f"groups must be offsets that run from 0 to B = {B} increasing (got {groups!r})")
    return np.ascontiguousarray(group_off, dtype=np.int32)


def refit_rows(rows, X, target, lengths=None, groups="pooled", free=None, max_iter: int = 50, gtol: float = 1e-10,
               xtol: float = 1e-12, variable_names=None, engine=None, device: bool = False) -> RowRefit:
    """Refit the constants of every row of ``rows`` to the derivative series ``target`` on the recordings X (T, F) or
    (B, T, F) of already-scaled feature rows (rovmpc_refit_rows; law in include/rovmpc.h): Levenberg-Marquardt on the `loss`
    column of ``score_rows``, all (row, group) problems in one launch.  ``groups``: "pooled" (one fit on all recordings),
    "each" (one per recording) or an offsets array 0 .. B; ``free``: per row a boolean sequence over the row's constants
    (default: all but those that occur only as POW exponents); ``lengths``: the rows of each recording that count.
    ``expressions`` are the rows with the returned constants written in (``rewrite_constants``).  The library never moves a
    constant that reaches a POW exponent (it refuses a free one), so an exponent keeps its value and ``x**2.5`` stays a POW;
    were a pool edited by hand so that such an exponent became a whole number, the text would compile to POWI, another
    operation sequence.  A start that is not a number is refused here, before the launch: it could not be written back."""
    if isinstance(rows, (str, dict)):
        raise ValueError("rows must be a sequence of rows, not a single row")
    texts = [row_text(r) for r in rows]
    if not texts:
        raise ValueError("rows is empty")
    if target is None:
        raise ValueError("target is required: the derivative series the constants are fitted to")
    X, _, target, _, lengths, _, _ = _recordings(X, target, target, None, lengths, None, names=("target", "target"))
    group_off = _group_offsets(groups, X.shape[0])
    params = _lib.RefitParams.make(max_iter, gtol, xtol)
    if free is not None and len(free) != len(texts):
        raise ValueError(f"free must hold one mask per row ({len(texts)}; got {len(free)})")
    programs, masks = [], []
    for r, text in enumerate(texts):
        consts: list = []
        prog = compile_expression(text, consts, X.shape[2], variable_names)
        if any(c != c for c in consts):
            raise ValueError(f"row {r} starts from a constant that is not a number: {text!r}")      # (it could not be written back)
        if free is None:
            mask = default_free(prog.code, len(consts), text)
        else:
            mask = np.asarray(free[r]).astype(bool).astype(np.uint8).reshape(-1)
            if mask.shape != (len(consts),):
                raise ValueError(f"free[{r}] must hold one flag per constant of the row ({len(consts)}; got {mask.shape[0]})")
        if int(mask.sum()) > _lib.REFIT_MAX_PARAMS:
            raise ValueError(f"row {r} has {int(mask.sum())} free constants (at most {_lib.REFIT_MAX_PARAMS}): freeze some with `free`")
        programs.append((prog.code, consts)); masks.append(mask)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    consts_out, out = engine.refit_rows(programs, X, target, lengths, group_off, masks, params, device)
    off = np.concatenate([[0], np.cumsum([len(k) for _, k in programs])]).astype(int)
    per_row = [np.ascontiguousarray(consts_out[:, off[r]:off[r + 1]]) for r in range(len(texts))]
    expressions = [[rewrite_constants(text, c, variable_names) for c in per_row[r]] for r, text in enumerate(texts)]
    col = lambda k, t=np.float64: np.ascontiguousarray(out[..., k]).astype(t)
    return RowRefit(per_row, expressions, col(0), col(1), col(2), col(3, np.int64), col(4, np.int64), col(5, np.int64))


class DiscoverStatus(enum.IntEnum):
    """``rovmpc_discover_status``: how the forward selection of ``discover_rows`` ended."""
    FULL = _lib.DISCOVER_FULL
    MIN_GAIN = _lib.DISCOVER_MIN_GAIN
    EXHAUSTED = _lib.DISCOVER_EXHAUSTED
    NONFINITE = _lib.DISCOVER_NONFINITE


def term_library(F: int, unary=("id", "sin", "cos"), intercept: bool = True, products=(), variable_names=None) -> list:
    """Term texts for ``discover_rows`` over F features, in this order: the intercept ``1.0`` (if asked for); then for every
    entry of ``unary`` in the order given, that function of every feature x0 .. x{F-1} in turn ("id" is the feature itself,
    the others the one-argument functions of the expression grammar: sin, cos, tanh, exp, ...); then ``x_i*x_j`` for every
    index pair of ``products`` in the order given.  F = 18 with the defaults: 1 + 3 * 18 = 55 texts.  ``variable_names``: the
    names written instead of x0 ...  More than 64 terms is an error: the library takes no more."""
    from .expr import _UNARY_CALLS
    if isinstance(F, bool) or int(F) != F or not 1 <= int(F) <= _lib.MAX_FEATURES:
        raise ValueError(f"F must be an integer in 1..{_lib.MAX_FEATURES} (got {F!r})")
    F = int(F)
    if variable_names is not None and len(variable_names) != F:
        raise ValueError(f"variable_names must hold F = {F} names (got {len(variable_names)})")
    name = (lambda i: variable_names[i]) if variable_names is not None else (lambda i: f"x{i}")
    terms = ["1.0"] if intercept else []
    for u in unary:
        if u != "id" and u not in _UNARY_CALLS:
            raise ValueError(f"unary must name 'id' or one of {sorted(_UNARY_CALLS)} (got {u!r})")
        terms += [name(i) if u == "id" else f"{u}({name(i)})" for i in range(F)]
    for pair in products:
        i, j = pair
        if not (0 <= int(i) < F and 0 <= int(j) < F):
            raise ValueError(f"a product names a feature outside 0..{F - 1} (got {pair!r})")
        terms.append(f"{name(int(i))}*{name(int(j))}")
    if len(terms) > _lib.DISCOVER_MAX_TERMS:
        raise ValueError(f"{len(terms)} terms: a library holds at most {_lib.DISCOVER_MAX_TERMS}")
    return terms


@dataclass
class RowFront:
    """What rovmpc_discover_rows returns for M terms on G groups with S = max_terms.  ``picks`` (G, S): the term of every
    step, -1 beyond ``n_sel``; ``coef`` (G, S, S): row s the coefficients of the size-(s+1) row in pick order; ``loss``
    (G, S + 1): loss[:, 0] is the mean square of the target, NaN beyond ``n_sel``; ``n_sel``, ``status``
    (``DiscoverStatus``), ``n`` (the counted rows), each (G,); ``terms``: the library's texts; ``gram`` (G, (M+1)(M+2)/2) where
    it was asked for.  ``expressions[g][s]``: the size-(s+1) row as text, ``a0*(t0) + a1*(t1) + ...`` with ``repr`` literals,
    for s < n_sel[g]; ``complexities[g][s]``: its compiled instruction count."""
    picks: np.ndarray
    coef: np.ndarray
    loss: np.ndarray
    n_sel: np.ndarray
    status: np.ndarray
    n: np.ndarray
    terms: Sequence[str]
    gram: Optional[np.ndarray] = None
    expressions: Sequence = ()
    complexities: Sequence = ()

    def rows(self, g: int = 0) -> list:
        """The front of group g as row dicts (``complexity``, ``loss``, ``equation``, ``sympy_format``), smallest first:
        what ``read_equation_csv`` returns for an equations_*.csv, and what ``score_rows``, ``refit_rows``, ``score_pairs``
        and ``select_model`` accept as they are.  ``complexity`` is the compiled row's instruction count, NOT PySR's
        complexity measure (which counts the nodes of its own expression tree)."""
        return [{"complexity": int(self.complexities[g][s]), "loss": float(self.loss[g, s + 1]), "equation": text, "sympy_format": text}
                for s, text in enumerate(self.expressions[g])]


def _front_texts(picks, coef, n_sel, terms, F, variable_names):
    """expressions[g][s] and their instruction counts; every text compiled once under the interpreter's limits."""
    expressions, complexities = [], []
    for g in range(len(picks)):
        texts, counts = [], []
        for s in range(int(n_sel[g])):
            text = " + ".join(f"{float(coef[g, s, i])!r}*({terms[int(picks[g, i])]})" for i in range(s + 1))
            try:
                prog = compile_expression(text, [], F, variable_names)
            except ValueError as e:
                raise ValueError(f"the size-{s + 1} row of group {g} does not compile: {e}") from None
            texts.append(text); counts.append(len(prog.code))
        expressions.append(texts); complexities.append(counts)
    return expressions, complexities


def discover_rows(terms, X, target, lengths=None, groups="pooled", max_terms: int = 8, dep_tol: float = 1e-10,
                  min_gain: float = 1e-12, variable_names=None, return_gram: bool = False, engine=None,
                  device: bool = False) -> RowFront:
    """Find equation rows on the recordings X (T, F) or (B, T, F) of already-scaled feature rows: for the sizes 1 ..
    ``max_terms`` the subset of ``terms`` (expression texts, e.g. ``term_library(F)``) whose linear combination fits the
    derivative series ``target`` best, by forward orthogonal least squares on the Gram matrix (rovmpc_discover_rows; law in
    include/rovmpc.h).  An intercept is the term ``"1.0"``; nothing is centred.  ``groups``: "pooled", "each" or an offsets
    array 0 .. B, one front per group; ``lengths``: the rows of each recording that count.  The selection stops before a
    term whose gain is at most ``min_gain`` times the target's sum of squares, and never takes a term whose part orthogonal
    to the picked ones is below ``dep_tol`` of its own square sum.  ``RowFront.rows()`` goes to ``score_rows``,
    ``refit_rows``, ``score_pairs`` and ``select_model`` as it is."""
    if isinstance(terms, (str, dict)):
        raise ValueError("terms must be a sequence of expression texts, not a single one")
    texts = [row_text(t) for t in terms]
    if not 1 <= len(texts) <= _lib.DISCOVER_MAX_TERMS:
        raise ValueError(f"1 to {_lib.DISCOVER_MAX_TERMS} terms (got {len(texts)})")
    if target is None:
        raise ValueError("target is required: the derivative series the rows are fitted to")
    X, _, target, _, lengths, _, _ = _recordings(X, target, target, None, lengths, None, names=("target", "target"))
    group_off = _group_offsets(groups, X.shape[0])
    params = _lib.DiscoverParams.make(max_terms, dep_tol, min_gain)
    programs = []
    for text in texts:
        consts: list = []
        prog = compile_expression(text, consts, X.shape[2], variable_names)
        programs.append((prog.code, consts))
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    picks, coef, loss, info, gram = engine.discover_rows(programs, X, target, lengths, group_off, params, return_gram, device)
    n_sel, status, n = (np.ascontiguousarray(info[:, k]) for k in range(3))
    expressions, complexities = _front_texts(picks, coef, n_sel, texts, X.shape[2], variable_names)
    return RowFront(picks, coef, loss, n_sel, status, n, tuple(texts), gram, expressions, complexities)


PREV_MODES = {"interp": _lib.PREV_INTERP, "hold": _lib.PREV_HOLD}
# metric -> whether larger is better ("skill": the mean of skill_theta and skill_gamma)
PAIR_METRICS = {"skill": True, "skill_theta": True, "skill_gamma": True, "coverage": True, "n_ok": True, "rmse_theta": False,
                "rmse_gamma": False, "max_abs_theta": False, "max_abs_gamma": False, "ss_theta": False, "ss_gamma": False}


@dataclass
class PairSkill:
    """What rovmpc_score_pairs returns for Q pairs on B recordings over H horizon steps.  ``pairs`` (Q, 2): theta row, gamma
    row; ``expressions[q]``: the pair's two texts; the nine columns each (Q, B, H); ``windows`` (B,): the windows W_b of each
    recording; ``pred`` (Q, B, W, H, 2) where it was asked for."""
    pairs: np.ndarray
    expressions: Sequence
    rmse_theta: np.ndarray
    rmse_gamma: np.ndarray
    max_abs_theta: np.ndarray
    max_abs_gamma: np.ndarray
    n_ok: np.ndarray
    ss_theta: np.ndarray
    ss_gamma: np.ndarray
    ss_hold_theta: np.ndarray
    ss_hold_gamma: np.ndarray
    windows: np.ndarray
    pred: Optional[np.ndarray] = None

    @classmethod
    def from_table(cls, table, pairs, expressions, windows, pred=None) -> "PairSkill":
        table = np.asarray(table, dtype=np.float64)
        if table.ndim != 4 or table.shape[3] != _lib.HORIZON_COLS:
            raise ValueError(f"skill must be (Q, B, H, {_lib.HORIZON_COLS}) (got {table.shape})")
        cols = [np.ascontiguousarray(table[..., k]) for k in range(_lib.HORIZON_COLS)]
        cols[4] = cols[4].astype(np.int64)
        return cls(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), tuple(expressions), *cols,
                   windows=np.asarray(windows, dtype=np.int64), pred=pred)

    def table(self) -> np.ndarray:
        return np.stack([np.asarray(getattr(self, n), dtype=np.float64) for n in _lib.HORIZON_NAMES], axis=-1)

    @staticmethod
    def _skill(ss, hold, n_ok):
        with np.errstate(all="ignore"):
            return np.where((hold == 0) | (n_ok == 0), np.nan, 1.0 - ss / hold)

    @property
    def skill_theta(self) -> np.ndarray:
        """1 - ss_theta / ss_hold_theta: 1 is perfect, 0 the persistence forecast; NaN where ss_hold = 0 or n_ok = 0."""
        return self._skill(self.ss_theta, self.ss_hold_theta, self.n_ok)

    @property
    def skill_gamma(self) -> np.ndarray:
        return self._skill(self.ss_gamma, self.ss_hold_gamma, self.n_ok)

    @property
    def skill(self) -> np.ndarray:
        return (self.skill_theta + self.skill_gamma) / 2

    @property
    def coverage(self) -> np.ndarray:
        """n_ok / W_b, the share of a recording's windows that were counted (NaN where it has none)."""
        with np.errstate(all="ignore"):
            return self.n_ok / np.where(self.windows > 0, self.windows, np.nan)[None, :, None]

    def rank(self, metric: str = "skill", at: Optional[int] = None, reduce: str = "mean") -> np.ndarray:
        """Pair indices, best first: the metric at horizon step ``at`` (1 .. H; default H, the last) reduced over the
        recordings (a NaN on any recording makes the pair's value NaN), NaN pairs last, ties to the lower index."""
        if metric not in PAIR_METRICS:
            raise ValueError(f"metric must be one of {sorted(PAIR_METRICS)} (got {metric!r})")
        if reduce not in REDUCERS:
            raise ValueError(f"reduce must be one of {REDUCERS} (got {reduce!r})")
        H = self.n_ok.shape[2]
        at = H if at is None else at
        if isinstance(at, bool) or int(at) != at or not 1 <= int(at) <= H:
            raise ValueError(f"at must be a horizon step in 1..{H} (got {at!r})")
        v = np.asarray(getattr(self, metric), dtype=np.float64)[:, :, int(at) - 1]
        with np.errstate(all="ignore"):
            v = getattr(np, reduce)(v, axis=1)
        key = -v if PAIR_METRICS[metric] else v
        key = np.where(np.isnan(key), np.inf, key)
        return np.lexsort((np.arange(len(v)), key, np.isnan(v))).astype(np.int64)

    def best(self, metric: str = "skill", at: Optional[int] = None, reduce: str = "mean") -> int:
        return int(self.rank(metric, at, reduce)[0])


def _pair_list(pairs, Rt: int, Rg: int) -> np.ndarray:
    if isinstance(pairs, str):
        if pairs == "product":
            return np.stack(np.meshgrid(np.arange(Rt), np.arange(Rg), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32)
        if pairs == "zip":
            if Rt != Rg:
                raise ValueError(f"pairs='zip' needs as many theta rows as gamma rows (got {Rt}, {Rg})")
            return np.stack([np.arange(Rt), np.arange(Rt)], axis=-1).astype(np.int32)
        raise ValueError(f"pairs must be 'product', 'zip' or a list of (theta row, gamma row) (got {pairs!r})")
    try:
        arr = np.asarray(pairs)
    except Exception:
        arr = None
    if arr is None or arr.ndim != 2 or arr.shape[1] != 2 or len(arr) < 1 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"pairs must be 'product', 'zip' or a non-empty list of integer (theta row, gamma row) (got {pairs!r})")
    if (arr < 0).any() or (arr[:, 0] >= Rt).any() or (arr[:, 1] >= Rg).any():
        raise ValueError(f"a pair is outside the fronts ({Rt} theta rows, {Rg} gamma rows)")
    return np.ascontiguousarray(arr, dtype=np.int32)


def score_pairs(theta_rows, gamma_rows, X, time, theta, gamma, mean, scale, horizon, stride: int = 1, pairs="product",
                integrator="rk4", prev_mode="interp", feature_map="gen1", lengths=None, variable_names=None,
                return_pred: bool = False, engine=None, device: bool = False) -> PairSkill:
    """Closed-loop N-step-ahead skill of (theta row, gamma row) pairs on recordings (rovmpc_score_pairs; law in
    include/rovmpc.h).  From every ``stride``-th row of a recording the pair is rolled ``horizon`` steps on its own
    predictions -- its (theta, gamma) written into the state slots of every RK4 stage row, the other slots taken from the
    recording -- and the error after 1 .. horizon steps is reduced over the windows, beside that of the persistence forecast.
    X (T, F) or (B, T, F): already-scaled feature rows; time, theta, gamma (T,) or (B, T): theta and gamma measured and
    UNSCALED; mean, scale (F,): the scaler (read at the state slots).  ``pairs``: "product" (every theta row with every gamma
    row, theta-major), "zip" or a list of (theta row, gamma row); ``feature_map``: "gen1" (slots 14, 15 and the delay slots
    16, 17), "gen2" (12, 13 and cos theta, sin gamma at 14, 15) or a dict {"theta", "gamma", "theta_prev", "gamma_prev",
    "cos_theta", "sin_gamma"} -> slot; ``integrator``: "rk4" or "euler"; ``prev_mode``: "interp" or "hold".  One launch."""
    if isinstance(integrator, str):
        if integrator not in ("rk4", "euler"):
            raise ValueError(f"integrator must be 'rk4' or 'euler' (got {integrator!r}; the second-order maps are not provided)")
        integrator = INTEGRATORS[integrator]
    if isinstance(prev_mode, str):
        if prev_mode not in PREV_MODES:
            raise ValueError(f"prev_mode must be one of {sorted(PREV_MODES)} (got {prev_mode!r})")
        prev_mode = PREV_MODES[prev_mode]
    if isinstance(feature_map, str):
        if feature_map not in _lib.FEATURE_MAPS:
            raise ValueError(f"feature_map must be one of {sorted(_lib.FEATURE_MAPS)} or a dict of slots (got {feature_map!r})")
        slots = _lib.FEATURE_MAPS[feature_map]
    elif isinstance(feature_map, dict):
        unknown = set(feature_map) - set(_lib.HORIZON_SLOTS)
        if unknown:
            raise ValueError(f"feature_map names {sorted(unknown)}; the slots are {_lib.HORIZON_SLOTS}")
        slots = tuple(-1 if feature_map.get(n) is None else feature_map[n] for n in _lib.HORIZON_SLOTS)
    else:
        raise ValueError(f"feature_map must be one of {sorted(_lib.FEATURE_MAPS)} or a dict of slots (got {feature_map!r})")
    fronts = []
    for name, rows in (("theta_rows", theta_rows), ("gamma_rows", gamma_rows)):
        if isinstance(rows, (str, dict)):
            raise ValueError(f"{name} must be a sequence of rows, not a single row")
        texts = [row_text(r) for r in rows]
        if not texts:
            raise ValueError(f"{name} is empty")
        fronts.append(texts)
    X, time, theta, gamma, lengths, _, _ = _recordings(X, time, theta, gamma, lengths, None, names=("time", "theta"))
    if gamma is None:
        raise ValueError("gamma is required")
    B, T, F = X.shape
    params = _lib.HorizonParams.make(horizon, stride, integrator, prev_mode, slots, F)
    mean, scale = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64)
    if mean.shape != (F,) or scale.shape != (F,):
        raise ValueError(f"mean and scale must be (F,) = ({F},) (got {mean.shape}, {scale.shape})")
    used = [v for v in params.slots() if v >= 0]
    if not np.isfinite(mean[used]).all() or not np.isfinite(scale[used]).all() or (scale[used] == 0).any():
        raise ValueError("mean and scale must be finite, the scale not 0, at the state slots")
    pair_arr = _pair_list(pairs, len(fronts[0]), len(fronts[1]))
    if len(pair_arr) * B > 1 << 24:
        raise ValueError(f"more than 2^24 (pair, recording) problems in one call (got {len(pair_arr)} x {B})")
    programs = []
    for texts in fronts:
        progs = []
        for text in texts:
            consts: list = []
            prog = compile_expression(text, consts, F, variable_names)
            progs.append((prog.code, consts))
        programs.append(progs)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    table, pred = engine.score_pairs(programs[0], programs[1], pair_arr, X, time, theta, gamma, mean, scale, params, lengths,
                                     return_pred, device)
    n = np.full(B, T, dtype=np.int64) if lengths is None else lengths
    H, stride = int(params.H), int(params.stride)
    windows = np.where(n - 1 - H >= 0, (n - 1 - H) // stride + 1, 0)
    expressions = [(fronts[0][it], fronts[1][ig]) for it, ig in pair_arr]
    return PairSkill.from_table(table, pair_arr, expressions, windows, pred)


def _derivative_target(series, time, lengths):
    """np.gradient(series, time) per recording over its counted rows (simply.py's target); 0 beyond them."""
    series, time = np.asarray(series, dtype=np.float64), np.asarray(time, dtype=np.float64)
    if series.shape != time.shape or series.ndim not in (1, 2):
        raise ValueError(f"series and time must both be (T,) or (B, T) (got {series.shape}, {time.shape})")
    s2, t2 = np.atleast_2d(series), np.atleast_2d(time)
    out = np.zeros_like(s2)
    for b in range(len(s2)):
        n = s2.shape[1] if lengths is None else int(np.asarray(lengths)[b])
        if n < 2:
            raise ValueError(f"recording {b} has {n} counted rows: a derivative needs at least 2")
        out[b, :n] = np.gradient(s2[b, :n], t2[b, :n])
    return out.reshape(series.shape)


def select_model(theta_rows, gamma_rows, X_raw, time, theta, gamma, mean, scale, integrator="rk4", metric: str = "r2",
                 reduce: str = "mean", lengths=None, variable_names=None, engine=None, refit: bool = False, horizon=None,
                 stride: int = 1, shortlist: int = 4):
    """Score both Pareto fronts on the recordings and return (the DynamicsModel of the two best rows, theta scores, gamma
    scores).  ``X_raw`` (T, F) or (B, T, F) are unscaled feature rows; they are scaled as the scaler does, (X - mean) / scale,
    before the rows read them.  ``theta`` / ``gamma``: the measured series the replays are held against.  ``refit=True``:
    the constants of both fronts are first refitted (``refit_rows``, all recordings pooled) to np.gradient(series, time), the
    reference's target (simply.py); the rewritten rows are scored -- with that target, so ``loss`` is theirs -- and loaded.
    ``horizon=H``: the open-loop ranking only shortlists.  The ``shortlist`` best rows of each front (refitted first with
    ``refit=True``) form shortlist^2 pairs, ``score_pairs`` rolls every pair H steps on its own predictions from every
    ``stride``-th row (generation-1 slots; "rk4" or "euler"), the pair with the best closed-loop skill at step H is loaded,
    and the PairSkill -- its ``pairs`` index the fronts' rows -- is returned as a fourth value."""
    if horizon is not None and (isinstance(shortlist, bool) or int(shortlist) != shortlist or int(shortlist) < 1):
        raise ValueError(f"shortlist must be an integer >= 1 (got {shortlist!r})")
    mean = np.asarray(mean, dtype=np.float64); scale = np.asarray(scale, dtype=np.float64)
    X_raw = np.asarray(X_raw, dtype=np.float64)
    if mean.ndim != 1 or mean.shape != scale.shape or X_raw.ndim not in (2, 3) or X_raw.shape[-1] != mean.shape[0]:
        raise ValueError(f"mean and scale must be (F,) with F = X_raw.shape[-1] (got {mean.shape}, {scale.shape}, {X_raw.shape})")
    Xs = (X_raw - mean) / scale
    kw = dict(integrator=integrator, lengths=lengths, variable_names=variable_names, engine=engine)
    if refit:
        fronts = []
        for rows, series in ((theta_rows, theta), (gamma_rows, gamma)):
            target = _derivative_target(series, time, lengths)
            fit = refit_rows(rows, Xs, target, lengths=lengths, variable_names=variable_names, engine=engine)
            fronts.append(score_rows([e[0] for e in fit.expressions], Xs, time, series, target=target, **kw))
        s_theta, s_gamma = fronts
    else:
        s_theta = score_rows(theta_rows, Xs, time, theta, **kw)
        s_gamma = score_rows(gamma_rows, Xs, time, gamma, **kw)
    if horizon is None:
        model = DynamicsModel(mean, scale, s_theta.expressions[s_theta.best(metric, reduce)],
                              s_gamma.expressions[s_gamma.best(metric, reduce)], variable_names=variable_names)
        return model, s_theta, s_gamma
    top_t, top_g = s_theta.rank(metric, reduce)[:int(shortlist)], s_gamma.rank(metric, reduce)[:int(shortlist)]
    skill = score_pairs([s_theta.expressions[r] for r in top_t], [s_gamma.expressions[r] for r in top_g], Xs, time, theta, gamma,
                        mean, scale, horizon, stride=stride, integrator=integrator, lengths=lengths, variable_names=variable_names,
                        engine=engine)
    skill.pairs = np.stack([top_t[skill.pairs[:, 0]], top_g[skill.pairs[:, 1]]], axis=-1)      # rows of the fronts, not of the shortlists
    it, ig = skill.pairs[skill.best(reduce=reduce)]
    model = DynamicsModel(mean, scale, s_theta.expressions[it], s_gamma.expressions[ig], variable_names=variable_names)
    return model, s_theta, s_gamma, skill
