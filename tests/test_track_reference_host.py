"""The tracker's reference on the CPU (tests/track_reference.py; law in include/rovmpc.h above rovmpc_track_markers): what the
recordings R1 .. R6 are expected to show, why per-frame cold fits are no substitute, the accepted frames against the 50-digit
minimiser within fit_reference's own margin, the split law, the conditions on R6's inputs, and five mutants of the law each
caught by a recording."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_reference as fr  # noqa: E402
import track_reference as tk  # noqa: E402

S, St = fr.Status, tk.State


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def by_name():
    return {r.name: (r, out, c) for r, (out, c) in zip(tk.recordings(), tk.references())}


def test_recordings_show_what_they_were_built_for():
    for rec, (out, c) in zip(tk.recordings(), tk.references()):
        states = tuple(St(int(x)) for x in out[:, 7])
        print(rec.name, [s.name for s in states], "starts", out[:, 8].astype(int), "steps", out[:, 5].astype(int))
        assert states == rec.states, rec.name
        for t, s in enumerate(states):
            row = out[t]
            if s in (St.LOCKED, St.ACQUIRED):
                assert S(int(row[6])) is S.CONVERGED and row[4] <= rec.rms_max and (row[8] == -1) == (s is St.LOCKED)
            else:
                assert np.isnan(row[4])
            if s is St.NONE:
                assert np.isnan(row[:4]).all()
            if s is St.HELD:
                assert same(row[0:2], row[2:4])                                # output = carry = what the frame found
    R = by_name()
    r1, o1, c1 = R["R1"]
    assert o1[0, 8] == 1                                                     # acquired from (0.3, 0), not from (0, 0)
    assert [S(int(x)) for x in o1[[5, 6, 9], 6]] == [S.TOO_FEW, S.TOO_FEW, S.NONFINITE]
    assert same(o1[5, 0:2], o1[4, 0:2]) and same(o1[6, 0:2], o1[4, 0:2]) and same(o1[9, 0:2], o1[8, 0:2])
    assert same(c1, o1[-1, 0:2])
    r2, o2, _ = R["R2"]
    assert r2.carry == (0.1, 0.5) and o2[0, 8] == -1 and same(o2[0, 2:4], r2.carry)
    assert same(o2[1:, 2:4], o2[:-1, 0:2])                                   # theta_prev, gamma_prev: the frame before
    r3, o3, _ = R["R3"]
    assert r3.M == 5 and r3.up == -1.0 and same(o3[0, 2:4], o3[0, 0:2])      # no carry: the frame's own angles
    _, o4, c4 = R["R4"]
    assert np.isnan(c4).all() and np.all(o4[:, 6] == S.TOO_FEW) and np.all(o4[:, 8] == 0)
    _, o5, c5 = R["R5"]
    assert len(o5) == 1 and same(c5, o5[0, 0:2])


def test_cold_fits_fail_on_r1():
    """The reason the tracker exists: from (0, 0), frame by frame, frames 0 .. 10 of R1 are CHORD, TOO_FEW or NONFINITE."""
    r1 = tk.recordings()[0]
    cold = [S(int(fr.fit_np(r1.A[t], r1.P[t], r1.Y[t])[5])) for t in range(len(r1.Y))]
    print([s.name for s in cold])
    assert all(s in (S.CHORD, S.TOO_FEW, S.NONFINITE) for s in cold[:11])
    assert sum(s is not S.CONVERGED for s in cold) == 11


def test_accepted_frames_against_the_50_digit_minimiser():
    n = 0
    for rec, (out, _), per in zip(tk.recordings(), tk.references(), tk.minimisers()):
        for t, (m, scale) in per.items():
            ea = max(tk.angle_errors(out[t, 0], out[t, 1], m))
            assert ea <= fr.M_FIT * scale, (rec.name, t, ea, scale)
            n += 1
    assert n >= 35


def test_split_law():
    """A recording cut into calls that hand the carry on gives the rows and the carry of the one call."""
    for rec, (want, c_want) in zip(tk.recordings(), tk.references()):
        T = len(rec.Y)
        for cuts in ([0, 5, T] if T > 5 else [0, T], list(range(T + 1))):
            c, parts = rec.carry, []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                o, c = tk.track_np(rec.A[lo:hi], rec.P[lo:hi], rec.Y[lo:hi], c, rec.starts, rec.rms_max, rec.up)
                parts.append(o)
            assert same(np.concatenate(parts), want) and same(c, c_want), (rec.name, cuts)
    r1 = tk.recordings()[0]
    assert same(tk.track_np(r1.A, r1.P, r1.Y, (np.nan, 0.2))[0], tk.references()[0][0])   # a half-finite carry is none


def test_r6_inputs_meet_their_conditions():
    """Every noise frame is below the 5 mm gate, and the displaced marker lifts its frame above it from every start."""
    rec, out, _ = by_name()["R6"]
    assert rec.rms_max == tk.R6_GATE
    for t in range(len(rec.Y)):
        if t != tk.R6_OUTLIER:
            assert out[t, 4] < tk.R6_GATE, (t, out[t, 4])
    t = tk.R6_OUTLIER
    carry = out[t - 1, 0:2]
    converged = 0
    for start in (tuple(carry),) + rec.starts:
        r = fr.fit_np(rec.A[t], rec.P[t], rec.Y[t], start, up=rec.up)
        print(start, S(int(r[5])).name, r[2])
        if S(int(r[5])) is S.CONVERGED:
            converged += 1
            assert r[2] > tk.R6_GATE
    assert converged >= 2 and S(int(fr.fit_np(rec.A[t], rec.P[t], rec.Y[t], carry, up=rec.up)[5])) is S.CONVERGED


MUTANTS = {"list-first": ("R1", {}), "no-hold": ("R1", {}), "accepts-max-iter": ("R5", {"max_iter": 2}),
           "carries-rejected": ("R6", {}), "ignores-rms-max": ("R6", {})}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_are_caught(mutant):
    name, kw = MUTANTS[mutant]
    rec = by_name()[name][0]
    law, _ = tk.track_np(rec.A, rec.P, rec.Y, rec.carry, rec.starts, rec.rms_max, rec.up, **kw)
    got, _ = tk.track_np(rec.A, rec.P, rec.Y, rec.carry, rec.starts, rec.rms_max, rec.up, mutant=mutant, **kw)
    states = lambda o: [St(int(x)).name for x in o[:, 7]]
    print(mutant, states(law), states(got))
    assert not same(got, law)
    if mutant == "no-hold":
        assert states(got)[5] == "NONE" and states(law)[5] == "HELD"
    if mutant == "accepts-max-iter":
        assert states(law) == ["NONE"] and states(got) == ["ACQUIRED"] and got[0, 6] == S.MAX_ITER
    if mutant == "ignores-rms-max":
        assert states(got)[tk.R6_OUTLIER] == "LOCKED" and states(law)[tk.R6_OUTLIER] == "HELD"
    if mutant == "carries-rejected":
        assert not same(got[tk.R6_OUTLIER + 1, 2:4], law[tk.R6_OUTLIER + 1, 2:4])
    if mutant == "list-first":
        assert np.any(got[1:, 8] != law[1:, 8]) or np.any(got[1:, 5] != law[1:, 5])


def test_no_mutant_changes_the_law_itself():
    for rec, (want, c) in zip(tk.recordings(), tk.references()):
        out, c2 = tk.track_np(rec.A, rec.P, rec.Y, rec.carry, rec.starts, rec.rms_max, rec.up, mutant=None)
        assert same(out, want) and same(c, c2)
    assert math.isinf(tk.recordings()[0].rms_max)
