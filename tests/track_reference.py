"""Reference of the marker tracker (law: include/rovmpc.h above rovmpc_track_markers): `track_np`, the plain restatement of
the chain on fit_reference.fit_np, and the recordings R1 .. R6 both the host test and the GPU test run.  The markers are
built the way fit_reference.make_frame builds them: the cable's points at 50 digits, rounded to fp64.

tests/test_track_reference_host.py checks the recordings' expectations and conditions on the CPU; tests/test_track_gpu.py
holds the kernel to the chain law bit for bit and to track_np's decisions."""
import collections
import enum
import functools
import math

import numpy as np
from mpmath import mp

import cable_reference as cr
import fit_reference as fr
import tether_reference as tr

OUT = 9
MAX_STARTS = 8
STARTS = ((0.0, 0.0), (0.3, 0.0), (-0.3, 0.0), (0.6, 0.0), (-0.6, 0.0))
S = fr.Status


class State(enum.IntEnum):
    LOCKED = 0
    ACQUIRED = 1
    HELD = 2
    NONE = 3


_memo = {}


def fit_cached(A, P, Y, guess, up, tol, max_iter):
    """fit_reference.fit_np, remembered per (frame, start, parameters): the chain, its split runs and its mutants ask for
    the same fits again and again."""
    key = (A.tobytes(), P.tobytes(), Y.tobytes(), float(guess[0]).hex(), float(guess[1]).hex(), up, tol, max_iter)
    if key not in _memo:
        _memo[key] = fr.fit_np(A, P, Y, guess, up=up, tol=tol, max_iter=max_iter)
    return _memo[key]


def track_np(A, P, Y, carry=None, starts=STARTS, rms_max=math.inf, up=1.0, tol=fr.TOL, max_iter=fr.MAX_ITER, mutant=None):
    """The law for one recording: A, P (T, 3), Y (T, M, 3), carry (2,) or None.  Returns (out (T, 9), outgoing carry (2,)).
    `mutant` names one deliberate departure from the law (test_track_reference_host.py shows each is caught)."""
    A, P, Y = (np.asarray(x, dtype=np.float64) for x in (A, P, Y))
    c = np.full(2, np.nan) if carry is None else np.array(carry, dtype=np.float64)
    out = np.empty((len(Y), OUT))
    for t in range(len(Y)):
        have = bool(np.isfinite(c).all())
        if not have:
            c = np.full(2, np.nan)
        attempts = ([(-1, c)] if have else []) + [(k, np.asarray(s, dtype=np.float64)) for k, s in enumerate(starts)]
        if mutant == "list-first" and have:
            attempts = attempts[1:] + attempts[:1]
        steps, accepted = 0, False
        for k, start in attempts:
            r = fit_cached(A[t], P[t], Y[t], start, up, tol, max_iter)
            steps += int(r[4])
            status = S(int(r[5]))
            good = (S.CONVERGED, S.MAX_ITER) if mutant == "accepts-max-iter" else (S.CONVERGED,)
            accepted = status in good and (r[2] <= rms_max or mutant == "ignores-rms-max")
            if accepted or status in (S.TOO_FEW, S.NONFINITE):
                break
        if accepted:
            state, th, ga = (State.LOCKED if k < 0 else State.ACQUIRED), r[0], r[1]
        elif have and mutant != "no-hold":
            state, th, ga = State.HELD, c[0], c[1]
        else:
            state, th, ga = State.NONE, np.nan, np.nan
        prev = c if have else (th, ga)
        out[t] = [th, ga, prev[0], prev[1], r[2] if accepted else np.nan, steps, status, state, k]
        if accepted or (mutant == "carries-rejected" and status not in (S.NONFINITE,)):
            c = np.array([r[0], r[1]])
    return out, c


# ---- the recordings -----------------------------------------------------------------------------------------------------

Recording = collections.namedtuple("Recording", "name A P Y carry starts rms_max M up truth states")


def markers(A, P, th, ga, M=16, up=1.0):
    """The M cable points of (th, ga) between A and P at 50 digits, rounded to fp64 (fit_reference.make_frame's way)."""
    with mp.workdps(fr.DPS):
        Am, Pm = [fr._mp(x) for x in A], [fr._mp(x) for x in P]
        pts = tr.node_points(Am, Pm, th, ga, fr._mp(fr.L_WS), M, fr._mp(up), fr._mp(fr.BRACKET[0]), fr._mp(fr.BRACKET[1]))[0]
        return np.array([[float(Am[j] + p[j]) for j in range(3)] for p in pts])


def _record(name, A, P, truth, M=16, up=1.0, carry=None, starts=STARTS, rms_max=math.inf, states=None):
    T = len(truth)
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), (T, 3)).copy()
    P = np.asarray(P, dtype=np.float64)
    Y = np.array([markers(A[t], P[t], truth[t][0], truth[t][1], M, up) for t in range(T)])
    return Recording(name, A, P, Y, carry, tuple(starts), rms_max, M, up, np.asarray(truth, dtype=np.float64), states)


def _geom(i, up=1.0, A=(0.0, 0.0, 0.0)):
    g = cr.shape_geometry(fr.L_WS)[i]
    return np.asarray(A, dtype=np.float64) + np.array([g[0], g[1], up * g[2]])


L, A_, H = State.LOCKED, State.ACQUIRED, State.HELD
R6_OUTLIER = 4                                       # the frame of R6 whose marker 7 is displaced by 10 cm
R6_GATE = 5e-3


@functools.lru_cache(maxsize=None)
def recordings():
    """R1 .. R6, in that order."""
    # R1: a near-vertical chord; per-frame fits from (0, 0) fail, the chain does not.  Frames 5 and 6 lose every marker,
    # frame 9 has a NaN in P1.
    T = 14
    P = [(0.023 + 0.004 * t, 0.026 - 0.003 * t, 0.759 + 0.01 * t) for t in range(T)]
    r1 = _record("R1", (0, 0, 0), P, [(-0.35 + 0.012 * t, 0.38 * math.cos(0.25 * t)) for t in range(T)],
                 states=(A_, L, L, L, L, H, H, L, L, H, L, L, L, L))
    r1.Y[5:7] = np.nan
    r1.P[9, 1] = np.nan
    # R2: the steep geometry 18, fast angles, an incoming carry at the truth of frame 0
    T = 12
    r2 = _record("R2", (0, 0, 0), [_geom(18)] * T, [(0.1 + 0.08 * t, 0.5 - 0.1 * t) for t in range(T)], carry=(0.1, 0.5),
                 states=(L,) * T)
    # R3: five markers, NED, the anchor away from the origin, the vehicle moving
    T = 6
    P = [_geom(9, -1.0, fr.ANCHOR) + np.array([0.02 * t, -0.01 * t, 0.015 * t]) for t in range(T)]
    r3 = _record("R3", fr.ANCHOR, P, [(0.05 + 0.04 * t, -0.2 + 0.07 * t) for t in range(T)], M=5, up=-1.0, states=(A_,) + (L,) * 5)
    # R4: no markers at all
    r4 = _record("R4", (0, 0, 0), [_geom(6)] * 3, [fr.truth_of(6)] * 3, states=(State.NONE,) * 3)
    r4.Y[:] = np.nan
    # R5: one frame
    r5 = _record("R5", (0, 0, 0), [_geom(6)], [fr.truth_of(6)], states=(A_,))
    # R6: geometry 6 with 1 mm noise under a 5 mm gate; one frame with an interior marker 10 cm off
    T = 8
    t6 = fr.truth_of(6)
    r6 = _record("R6", (0, 0, 0), [_geom(6)] * T, [(t6[0] + 0.01 * t, t6[1] - 0.015 * t) for t in range(T)], rms_max=R6_GATE,
                 states=tuple(H if t == R6_OUTLIER else (A_ if t == 0 else L) for t in range(T)))
    r6.Y[:, 1:-1] += 1e-3 * np.random.default_rng(606).standard_normal((T, 14, 3))
    r6.Y[R6_OUTLIER, 7] += np.array([0.06, -0.06, 0.05291502622129181])          # |d| = 0.1 m
    return r1, r2, r3, r4, r5, r6


@functools.lru_cache(maxsize=None)
def references():
    """track_np's (out, carry) per recording."""
    return tuple(track_np(r.A, r.P, r.Y, r.carry, r.starts, r.rms_max, r.up) for r in recordings())


def frame_of(rec, t):
    """Frame t of a recording as a fit_reference.Frame (for scale_of and fit_mp)."""
    return fr.Frame(f"{rec.name}[{t}]", None, rec.A[t], rec.P[t], rec.Y[t], None, rec.M, rec.up, fr.MAX_ITER, tuple(rec.truth[t]), False)


@functools.lru_cache(maxsize=None)
def minimisers():
    """Per recording and accepted frame of its reference: (the 50-digit minimiser from the truth, the error scale s)."""
    out = []
    for rec, (ref, _) in zip(recordings(), references()):
        per = {}
        for t in range(len(rec.Y)):
            if State(int(ref[t, 7])) in (State.LOCKED, State.ACQUIRED):
                f = frame_of(rec, t)
                m = fr.fit_mp(f.A, f.P, f.Y, f.truth, up=f.up)
                sigma = float(np.linalg.svd(m.J, compute_uv=False)[-1])
                per[t] = (m, fr.scale_of(f, m.kappa, sigma))
        out.append(per)
    return tuple(out)


def angle_errors(theta, gamma, m):
    with mp.workdps(fr.DPS):
        return float(abs(fr._mp(theta) - m.theta)), float(abs(fr._mp(gamma) - m.gamma))
