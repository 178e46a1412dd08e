"""The 50-digit reference of the tether keep-out cost (tests/tether_reference.py) on the CPU: the margin M_TETHER measured
with the plain fp64 NumPy restatement over every scene the GPU test runs, the conditions those scenes must meet so that no
case is left out, and the reference's own pieces against the cable reference and against closed forms."""
import os
import sys

import numpy as np
import pytest
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cable_reference as cr  # noqa: E402
import tether_reference as tr  # noqa: E402

CASES = [(N, K, M, 1.0) for N, K, M in tr.SHAPES] + [tr.FRAMES_AT + (-1.0,)]


def as_float(a):
    return np.array([[[float(x) for x in row] for row in cand] for cand in a])


def test_margin_is_measured_by_the_numpy_restatement():
    """m = twice the largest error-to-scale ratio of tether_np against the reference, never below 4; the restatement must
    stay inside m / 2.  Also: with 1 and 3 spheres (prefixes of the 8) the restatement agrees as well."""
    worst_D = worst_C = 0.0
    for N, K, M, up in CASES:
        sc, ref8 = tr.scene_reference(N, K, M, up)
        for n_sph in (1, 3, 8):
            ref = tr.prefix(ref8, n_sph)
            sph = sc.spheres[:n_sph]
            C, D = tr.tether_np(sc.state, sc.U, sc.traj, sph, tr.W, tr.MARGIN, M=M, up=up)
            rD, rC = tr.ratios(C, D, ref, sc.state, sph, tr.W)
            print(f"N {N} K {K} M {M} up {up:+.0f} {n_sph} spheres: largest error / scale: D {rD:.3g}, C {rC:.3g}")
            worst_D, worst_C = max(worst_D, rD), max(worst_C, rC)
    print(f"largest ratios: distance {worst_D:.4g}, C {worst_C:.4g}; M_TETHER = {tr.M_TETHER}")
    assert tr.M_TETHER >= 4.0
    assert max(worst_D, worst_C) <= tr.M_TETHER / 2
    assert tr.M_TETHER <= max(4.0, 2.2 * max(worst_D, worst_C))              # and not wider than the protocol gives


def test_prefix_equals_a_reference_of_its_own():
    N, K, M = 2, 5, 3
    sc, ref8 = tr.scene_reference(N, K, M)
    own = tr.tether_ref(sc.state, sc.U, sc.traj, sc.spheres[:3], tr.W, tr.MARGIN, M=M)
    pre = tr.prefix(ref8, 3)
    assert list(own.C) == list(pre.C) and np.array_equal(own.D, pre.D) and np.array_equal(own.pen, pre.pen)


def test_scene_conditions():
    """What the scenes must hold so that every node is decided and every path of the law is met."""
    sizes = 0
    for N, K, M, up in CASES:
        sc, ref = tr.scene_reference(N, K, M, up)
        # built for the engine bracket (1e-6, 200); values exact in float32, so one reference serves both dtypes
        assert tr.BRACKET == (1e-6, 200.0)
        for a in (sc.U, sc.traj):
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
        # no root within 1e-3 (relative) of a bracket end: nothing is undecided
        rc = ref.rootC[np.isfinite(ref.rootC)]
        for end in tr.BRACKET:
            assert np.all(np.abs(rc - end) > 1e-3 * end), (N, K, M, end)
        # chord exactly where there is no root in the bracket
        with np.errstate(invalid="ignore"):
            inside = np.isfinite(ref.rootC) & (ref.rootC >= tr.BRACKET[0]) & (ref.rootC <= tr.BRACKET[1])
        assert np.array_equal(ref.chord, ~inside)
        pen = as_float(ref.pen)
        clear = as_float(ref.clear)
        assert np.all(np.isfinite(pen))
        for n_sph in (1, 3, 8):
            assert (pen[:, :, :n_sph] > 0).mean() >= 0.2, (N, K, M, n_sph)
        assert np.all(pen[:, :, 0] > 0)                                        # sphere 0 contains the anchor
        a = sc.spheres[0]
        assert np.linalg.norm(a[:3] - sc.state[0:3]) < a[3]
        sizes += pen.size
        if N * K >= 10:
            assert np.any((pen == 0) & (clear > 0)), (N, K, M)                 # pen exactly 0, further than the margin away
            assert ref.chord.any(), (N, K, M)
        # a vertical rel (degenerate xy projection) at node 1 of candidate 0
        P = tr.C_STEP * sc.U[0, 0] + sc.state[3:6]
        rel = P - sc.state[0:3]
        assert rel[0] == 0.0 and rel[1] == 0.0 and rel[2] != 0.0
    # beyond taut among the chords, and a very slack cable whose root lies beyond c_hi
    sc, ref = tr.scene_reference(11, 67, 16)
    assert np.any(ref.chord & np.isnan(ref.rootC)) and np.any(ref.chord & (ref.rootC > tr.BRACKET[1]))
    print("triples checked:", sizes)


def test_node_points_against_the_cable_reference():
    """The lowest of a node's points is cable_reference.lowest_z_true, and its ends are the anchor and the vehicle."""
    with mp.workdps(tr.DPS):
        Af = [0.25, -0.5, 0.75]
        A = [mpf(a) for a in Af]
        for i, (rel, th, ga, M, up) in enumerate(cr.shape_cases()[::7]):
            Pf = [Af[j] + rel[j] for j in range(3)]                            # the doubles both references receive
            P = [mpf(p) for p in Pf]
            rel = [P[j] - A[j] for j in range(3)]
            pts, kap, C, chord = tr.node_points(A, P, th, ga, mpf(3.0), M, mpf(up), mpf(tr.BRACKET[0]), mpf(tr.BRACKET[1]))
            low = cr.lowest_z_true(Af, Pf, th, ga, 3.0, M, up, *tr.BRACKET)
            zs = [up * (A[2] + p[2]) for p in pts]
            assert abs(up * min(zs) - low.z) < mpf(10) ** -40, i
            assert chord == (not low.valid) and kap == low.kappa
            assert all(abs(x) < mpf(10) ** -45 for x in pts[0])
            assert all(abs(pts[-1][j] - rel[j]) < mpf(10) ** -40 for j in range(3)), i


def test_cable_distance_closed_forms():
    with mp.workdps(tr.DPS):
        pts = [[mpf(0), mpf(0), mpf(0)], [mpf(1), mpf(0), mpf(0)], [mpf(1), mpf(1), mpf(0)], [mpf(1), mpf(1), mpf(0)]]   # one zero-length segment
        assert tr.cable_distance(pts, [mpf("0.5"), mpf(0), mpf(2)]) == 2                     # above the middle of segment 0
        assert tr.cable_distance(pts, [mpf(-3), mpf(0), mpf(4)]) == 5                        # beyond the first end: t* = 0
        assert tr.cable_distance(pts, [mpf(1), mpf(4), mpf(-4)]) == 5                        # beyond the last end: t* = 1
        assert tr.cable_distance(pts, [mpf(1), mpf("0.25"), mpf(0)]) == 0                    # on the cable


def test_nonfinite_nodes():
    sc = tr.scene(2, 5, 3)
    traj = sc.traj.copy()
    traj[1, 2, 0] = np.nan
    traj[3, 1, 1] = np.inf
    U = sc.U.copy()
    U[4, 0] = (sc.state[0:3] - sc.state[3:6]) / tr.C_STEP                     # (not exact: rel = 0 is planted below instead)
    ref = tr.tether_ref(sc.state, sc.U, traj, sc.spheres[:2], tr.W, tr.MARGIN, M=3)
    C, D = tr.tether_np(sc.state, sc.U, traj, sc.spheres[:2], tr.W, tr.MARGIN, M=3)
    assert ref.C[1] == mp.inf and ref.C[3] == mp.inf and mp.isnan(ref.D[1, 1]) and mp.isnan(ref.D[3, 0])
    assert mp.isfinite(ref.D[1, 0]) and mp.isfinite(ref.D[3, 1]) and all(mp.isfinite(ref.C[k]) for k in (0, 2, 4))
    eC, eD = tr.errors(C, D, ref)
    assert np.all(np.isfinite(eC)) and np.all(np.isfinite(eD))
    # rel = 0: the vehicle at the anchor
    st = sc.state.copy()
    st[3:6] = st[0:3]
    ref0 = tr.tether_ref(st, np.zeros((1, 1, 3)), sc.traj[:1, :2], sc.spheres[:1], tr.W, tr.MARGIN, M=3)
    C0, D0 = tr.tether_np(st, np.zeros((1, 1, 3)), sc.traj[:1, :2], sc.spheres[:1], tr.W, tr.MARGIN, M=3)
    assert ref0.C[0] == mp.inf and C0[0] == np.inf and np.isnan(D0[0, 0])
