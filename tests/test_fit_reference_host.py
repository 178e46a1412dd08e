"""The 50-digit reference of the marker fit (tests/fit_reference.py) on the CPU: the margin M_FIT measured with the plain fp64
NumPy restatement over every scene the GPU test runs, the conditions those scenes must meet so that the GPU test cannot pass
by conditioning alone, the reference's model against the tether reference, and the alias of a steep chord."""
import os
import sys

import numpy as np
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cable_reference as cr  # noqa: E402
import fit_reference as fr  # noqa: E402
import tether_reference as tr  # noqa: E402

S = fr.Status


def test_margin_is_measured_by_the_numpy_restatement():
    """m = twice the largest error-to-scale ratio of fit_np against the 50-digit minimiser (angles over s, rms over s |J|),
    never below 4; the restatement must stay inside m / 2."""
    worst_a = worst_r = 0.0
    for f, r in zip(fr.scenes(), fr.references()):
        if r.mp is None:
            continue
        ea = max(fr.angle_errors(r.np_out[0], r.np_out[1], r)) / r.scale
        er = fr.rms_error(r.np_out[2], r)[0] / (r.scale * r.jnorm)
        print(f"{f.name:16s} trial steps {int(r.np_out[4]):2d} sigma {r.sigma:.3f} |J| {r.jnorm:.2f} kappa' {r.mp.kappa:7.1f} s {r.scale:.2e}: "
              f"error / scale: angle {ea:.3g}, rms {er:.3g}")
        worst_a, worst_r = max(worst_a, ea), max(worst_r, er)
    print(f"largest ratios: angle {worst_a:.4g}, rms {worst_r:.4g}; M_FIT = {fr.M_FIT}")
    assert fr.M_FIT >= 4.0
    assert max(worst_a, worst_r) <= fr.M_FIT / 2
    assert fr.M_FIT <= max(4.0, 2.2 * max(worst_a, worst_r))                 # and not wider than the protocol gives


def test_scene_conditions():
    scenes, refs = fr.scenes(), fr.references()
    assert len(scenes) <= 80
    assert fr.BRACKET == (1e-6, 200.0)
    # every status value occurs, and three quarters of the frames converge
    assert {r.status for r in refs} == set(S)
    assert sum(r.status is S.CONVERGED for r in refs) >= 0.75 * len(refs)
    expected = {"nonfinite-P": S.NONFINITE, "nonfinite-rel0": S.NONFINITE, "too-few": S.TOO_FEW, "chord": S.CHORD,
                "degenerate": S.DEGENERATE, "max-iter": S.MAX_ITER}
    n_noisy = 0
    for f, r in zip(scenes, refs):
        assert r.status is expected.get(f.name, S.CONVERGED), f.name
        assert r.np_out[4] <= f.max_iter
        if r.status is not S.CONVERGED:
            continue
        assert r.mp is not None, f.name
        # no root within 1e-3 (relative) of a bracket end: nothing is undecided
        for end in fr.BRACKET:
            assert abs(r.mp.rootC - end) > 1e-3 * end, (f.name, end)
        if f.noisy:
            n_noisy += 1
            assert 5e-4 < float(r.mp.rms) < 3e-3, f.name
        else:
            # the test cannot pass by conditioning alone
            assert fr.M_FIT * r.scale < 1e-9, (f.name, r.scale)
            assert r.sigma >= 0.16, (f.name, r.sigma)
            # the markers are the truth's to rounding: so is the minimiser
            assert max(abs(float(r.mp.theta) - f.truth[0]), abs(float(r.mp.gamma) - f.truth[1])) <= r.scale, f.name
    assert n_noisy == 8
    # the shapes: M = 3 and 5, both frames, an anchor off the origin, missing markers with both ends missing
    assert {f.M for f in scenes} == {3, 5, 16}
    assert sum(f.up < 0 for f in scenes) == 4 and sum(bool(f.A.any()) and f.truth is not None for f in scenes) == 4
    missing = sorted(int(np.isnan(f.Y).any(axis=1).sum()) for f in scenes if f.name.startswith("g") and "miss" in f.name)
    assert missing == [1, 5, 13]
    assert any(np.isnan(f.Y[0]).any() and np.isnan(f.Y[-1]).any() and r.status is S.CONVERGED for f, r in zip(scenes, refs))


def test_non_iterating_statuses_return_the_start():
    for f, r in zip(fr.scenes(), fr.references()):
        if r.status in (S.TOO_FEW, S.CHORD, S.DEGENERATE):
            g = (0.0, 0.0) if f.guess is None else f.guess
            assert r.np_out[0] == g[0] and r.np_out[1] == g[1] and r.np_out[4] == 0 and r.np_out[2] == r.np_out[3], f.name
        if r.status is S.NONFINITE:
            assert np.isnan(r.np_out[:4]).all() and r.np_out[4] == 0


def test_model_against_the_tether_reference():
    """points_mp at double angles is tether_reference.node_points; model_np agrees with it to the tether scale."""
    with mp.workdps(fr.DPS):
        A = [mpf(0)] * 3
        for i in (0, 6, 13, 18, 20, 21):
            g = cr.shape_geometry()[i]
            P = [mpf(x) for x in g]
            th, ga = fr.truth_of(i)
            args = (mpf(fr.L_WS), 16, mpf(1), mpf(fr.BRACKET[0]), mpf(fr.BRACKET[1]))
            want = tr.node_points(A, P, th, ga, *args)
            got = fr.points_mp(A, P, mpf(th), mpf(ga), *args)
            assert got[0] == want[0] and got[1:] == want[1:], i
            X, flag, _ = fr.model_np(np.array(g), th, ga, fr.L_WS, 16, 1.0, fr.BRACKET)
            assert flag == (0.0 if want[3] else 1.0), i
            err = max(abs(float(mpf(X[m, j]) - want[0][m][j])) for m in range(16) for j in range(3))
            assert err <= tr.M_TETHER * fr.EPS * (1.0 + want[1]) * fr.L_WS, (i, err)


def test_steep_chord_alias():
    """Geometry 18 (elevation -1.5) from (0, 0): the fit ends at another pair of angles than the truth's with a residual at
    rounding level -- two angle pairs, one curve."""
    f = fr.make_frame("g18", 18)
    row = fr.fit_np(f.A, f.P, f.Y, (0.0, 0.0))
    assert fr.Status(int(row[5])) is S.CONVERGED
    assert abs(row[0] - f.truth[0]) > 0.1 and abs(row[1] - f.truth[1]) > 1.0, row
    assert row[2] < 1e-14
    with mp.workdps(fr.DPS):
        args = ([mpf(0)] * 3, [mpf(float(x)) for x in f.P])
        tail = (mpf(fr.L_WS), 16, mpf(1), mpf(fr.BRACKET[0]), mpf(fr.BRACKET[1]))
        one = tr.node_points(*args, f.truth[0], f.truth[1], *tail)[0]
        two = tr.node_points(*args, float(row[0]), float(row[1]), *tail)[0]
        gap = max(abs(float(one[m][j] - two[m][j])) for m in range(16) for j in range(3))
    print(f"truth {f.truth}, alias ({row[0]:.6f}, {row[1]:.6f}), largest distance between the two curves' samples {gap:.3g} m")
    assert gap < 1e-13
