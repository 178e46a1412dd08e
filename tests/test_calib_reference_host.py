"""Host-side checks of the cable-length calibration's reference (tests/calib_reference.py): the NumPy restatement against the
50-digit law (these runs are where the allowances of tests/golden/calib_bounds.json were measured: each test re-measures its
figure and holds the record to it), the stored 50-digit minimiser's stationarity, and the host side of
rovmpc.calibrate_cable through a stand-in engine that answers with calib_np.  No GPU."""
import ctypes as C
import dataclasses
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_reference as cf  # noqa: E402
import fit_reference as fr  # noqa: E402

import rovmpc  # noqa: E402


def held(name, measured):
    """The record is this measurement (taken where the file was written; another libm may move it: a factor 2 up, 4 down)."""
    rec = cf.bounds()[name]
    print(f"{name}: measured {measured:.4g}, recorded {rec:.4g}")
    assert measured <= 2.0 * rec and rec <= 4.0 * measured, (name, measured, rec)


def test_forward_model_restatement_against_50_digits():
    from mpmath import mp
    worst = 0.0
    for M in cf.FORWARD_M:
        for arc in (cf.uniform_arc(M), cf.uneven_arc(M)):
            for name, A, P, th, ga, L in cf.forward_cases():
                X = cf.markers_np(A, P, th, ga, L, arc, M)[0]
                if name == "nan-angle":
                    assert np.isnan(X).all()
                    continue
                ref, chord = cf.markers_mp(A, P, th, ga, L, arc, M)
                assert chord == (name == "chord"), name
                with mp.workdps(cf.DPS):
                    worst = max(worst, max(float(abs(cf._mp(X[m, i]) - ref[m][i])) for m in range(M) for i in range(3)) / (cf.EPS * L))
    held("forward_np_max_err_uL", worst)


def test_cases_are_what_they_claim():
    from mpmath import mp, mpf
    by = {c[0]: c for c in cf.forward_cases()}
    with mp.workdps(cf.DPS):
        for name in ("steep-up", "steep-down"):
            _, A, P, th, ga, L = by[name]
            assert 0.85 <= abs(P[2] - A[2]) / L <= 0.95
        _, A, P, th, ga, L = by["taut"]
        assert 0.98 * L <= np.linalg.norm(P - A) < L
        _, A, P, th, ga, L = by["slack"]
        rel = [cf._mp(x) for x in P - A]
        Bp = cf.cr._rod(rel, cf.cr._axes(rel)[0], cf._mp(th))
        C = cf.cr._root_mp(mp.sqrt(Bp[0] ** 2 + Bp[1] ** 2), Bp[2], mpf(L))[1]
        assert 0.75 * cf.BRACKET[1] <= C <= cf.BRACKET[1], float(C)
        assert np.linalg.norm(by["chord"][2] - by["chord"][1]) > by["chord"][5]


def test_placement_inverts_the_arc_integral():
    _, A, P, th, ga, L = cf.forward_cases()[1]
    from mpmath import mp
    for s in (0.25, 0.7):
        t = cf.chord_parameter_mp(A, P, th, ga, L, s)
        with mp.workdps(cf.DPS):
            assert abs(cf.arc_integral_mp(A, P, th, ga, L, t) - cf._mp(s) * cf._mp(L)) < 1e-30


def test_asinh_restatement_through_the_placement():
    from mpmath import mp
    M = len(cf.ASINH_ARC)
    worst, lo, hi = 0.0, np.inf, 0.0
    for case in cf.asinh_cases():
        A, P, th, ga, L, bracket, _ = case
        X = cf.markers_np(A, P, th, ga, L, cf.ASINH_ARC, M, bracket=bracket, root_C=cf.asinh_root(case))[0]
        ref, chord = cf.markers_mp(A, P, th, ga, L, cf.ASINH_ARC, M, bracket=bracket)
        assert not chord
        xs, kappa = cf.asinh_arguments(case)
        lo, hi = min(lo, min(x for x in xs if x > 0)), max(hi, max(xs))
        with mp.workdps(cf.DPS):
            worst = max(worst, max(float(abs(cf._mp(X[m, i]) - ref[m][i])) for m in range(M) for i in range(3)) / (cf.EPS * L * (1.0 + kappa)))
    assert lo <= 2.0 ** -60 and hi >= np.e ** 16, (lo, hi)
    held("asinh_np_max_err_uL", worst)
    # and the function alone against mpmath over |x| from 2^-60 to e^16
    x = np.concatenate([2.0 ** np.arange(-60, 24, 0.37), -(2.0 ** np.arange(-60, 24, 0.37)), [0.0, np.e ** 16]])
    with mp.workdps(cf.DPS):
        err = max(abs(float((cf._mp(v) - mp.asinh(cf._mp(float(xi)))) / (mp.asinh(cf._mp(float(xi))) or 1))) for xi, v in zip(x, cf.asinh_np(x)))
    assert err <= 4 * cf.EPS, err


def test_recovery_by_the_restatement():
    eL = ea = 0.0
    for L_true in (2.7, 3.3):
        for n, M in cf.RECOVERY_GROUPS:
            r = cf.recording(n, L_true, seed=n + M, M=M)
            o = cf.calib_np(r["P0"], r["P1"], r["Y"], r["guess"], r["arc"], L0=3.0)
            assert o.group[5] == cf.CONVERGED and 5 <= o.group[4] <= 6 and o.group[6] == n and o.group[7] == n * M, (L_true, n, M, o.group)
            eL = max(eL, abs(o.group[0] - L_true))
            ea = max(ea, np.abs(o.frames[:, 0] - r["theta"]).max(), np.abs(o.frames[:, 1] - r["gamma"]).max())
    held("recovery_np_max_err_L", eL)
    held("recovery_np_max_err_angle", ea)


def test_restatement_against_the_50_digit_law_on_small_cases():
    """Two small noisy groups: calib_np's estimate against the 50-digit joint minimiser from the same start."""
    from mpmath import mp
    for n, M, seed in ((3, 5, 11), (2, 16, 12)):
        r = cf.recording(n, 2.7, seed=seed, M=M, noise=1e-3)
        o = cf.calib_np(r["P0"], r["P1"], r["Y"], r["guess"], r["arc"], L0=3.0, tol=cf.NOISY_TOL, tol_L=cf.NOISY_TOL)
        m = cf.calib_mp(r["P0"], r["P1"], r["Y"], r["guess"][:, 0], r["guess"][:, 1], 3.0, r["arc"])
        assert o.group[5] == cf.CONVERGED
        with mp.workdps(cf.DPS):
            dL = float(abs(cf._mp(o.group[0]) - m.L))
            da = max(max(float(abs(cf._mp(o.frames[f, 0]) - m.theta[f])), float(abs(cf._mp(o.frames[f, 1]) - m.gamma[f]))) for f in range(n))
        print(f"{n} frames, M = {M}: trial steps {int(o.group[4])}, to the minimiser: L {dL:.3g}, angle {da:.3g}; sigma_L {o.group[3]:.3g}")
        assert dL <= 1e-10 and da <= 1e-10                                  # (the stop at 1e-9 leaves a quadratically smaller distance)


def test_noisy_case_and_its_stored_minimiser():
    from mpmath import mp, mpf
    with open(os.path.join(cf.GOLDEN, "calib_minimisers.json")) as f:
        gold = json.load(f)
    assert gold["case"] == cf.NOISY
    r = cf.recording(**cf.NOISY)
    assert np.isnan(r["Y"]).any()
    with mp.workdps(cf.DPS):
        m = cf.calib_mp(r["P0"], r["P1"], r["Y"], [mpf(t) for t in gold["theta"]], [mpf(g) for g in gold["gamma"]], mpf(gold["L"]), r["arc"],
                        steps=False)
    assert m.grad <= 1e-20, m.grad                                          # stationary: J^T r = 0 to 20 digits
    o = cf.calib_np(r["P0"], r["P1"], r["Y"], r["guess"], r["arc"], L0=3.0, tol=cf.NOISY_TOL, tol_L=cf.NOISY_TOL)
    assert o.group[5] == cf.CONVERGED and o.group[6] == cf.NOISY["n"]
    with mp.workdps(cf.DPS):
        dL = float(abs(cf._mp(o.group[0]) - mpf(gold["L"])))
        da = max(max(float(abs(cf._mp(o.frames[f, 0]) - mpf(gold["theta"][f]))), float(abs(cf._mp(o.frames[f, 1]) - mpf(gold["gamma"][f]))))
                 for f in range(len(o.frames)))
    held("noisy_np_distance_L", dL)
    held("noisy_np_distance_angle", da)
    ratio = abs(o.group[0] - cf.NOISY["L_true"]) / o.group[3]
    print(f"noisy: L^ {o.group[0]:.12f}, sigma_L {o.group[3]:.3g}, |L^ - L_true| = {ratio:.3g} sigma_L, trial steps {int(o.group[4])}")
    assert ratio <= 3.0                                                     # (seed 7 was picked so that this holds)


def test_one_frame_fixed_length_restatement_follows_the_fit():
    """The tie on the CPU: statuses and trial-step counts of calib_np equal fit_np's on every scene (the bits are the GPU's
    business: the two restatements vectorise differently)."""
    for f in fr.scenes():
        a = fr.fit_np(f.A, f.P, f.Y, f.guess, up=f.up, max_iter=f.max_iter)
        o = cf.calib_np(f.A[None], f.P[None], f.Y[None], None if f.guess is None else f.guess[None], None, L0=cf.L_WS, free_length=False,
                        max_iter=f.max_iter, up=f.up)
        assert o.frames[0, 4] == a[5] and o.group[4] == a[4], (f.name, o, a)
        if a[5] == fr.Status.CONVERGED:
            assert abs(o.frames[0, 0] - a[0]) <= 1e-10 and abs(o.frames[0, 1] - a[1]) <= 1e-10


# ---- the host side of rovmpc.calibrate_cable -----------------------------------------------------------------------------------

class StandInEngine:
    """Answers Engine.calibrate_cable with calib_np, group by group."""

    def __init__(self):
        self.calls = []

    def calibrate_cable(self, P0, P1, Y, group_off, guess=None, arc=None, L0=None, free_length=True, L_lo=0.0, L_hi=float("inf"),
                        tol=1e-12, tol_L=1e-12, max_iter=60, device=False):
        self.calls.append(dict(F=len(Y), off=np.array(group_off), guess=guess, arc=arc, L0=L0))
        og, of = [], np.full((len(Y), 5), np.nan)
        for a, b in zip(group_off[:-1], group_off[1:]):
            o = cf.calib_np(P0[a:b], P1[a:b], Y[a:b], None if guess is None else guess[a:b], arc, L0=3.0 if L0 is None else L0,
                            free_length=free_length, L_lo=L_lo, L_hi=L_hi, tol=tol, tol_L=tol_L, max_iter=max_iter)
            og.append(o.group)
            of[a:b] = o.frames
        return np.array(og), of


def test_calibrate_cable_shapes_and_groups():
    eng = StandInEngine()
    r = cf.recording(6, 2.7, seed=3)
    arc = r["arc"]
    one = rovmpc.calibrate_cable(r["P0"], r["P1"], r["Y"], guess=r["guess"], arc=arc, engine=eng)
    assert np.ndim(one.L) == 0 and one.theta.shape == (6,) and one.frame_status.dtype == np.int64 and int(one.status) == rovmpc.CalibStatus.CONVERGED
    assert abs(one.L - 2.7) < 1e-12 and int(one.n_active) == 6 and int(one.n_markers) == 96 and list(eng.calls[-1]["off"]) == [0, 6]
    Yb = np.stack([r["Y"][:3], r["Y"][3:]])
    P1b, gb = np.stack([r["P1"][:3], r["P1"][3:]]), np.stack([r["guess"][:3], r["guess"][3:]])
    two = rovmpc.calibrate_cable(np.zeros(3), P1b, Yb, guess=gb, arc=arc, engine=eng)
    assert two.L.shape == (2,) and two.theta.shape == (2, 3) and list(eng.calls[-1]["off"]) == [0, 3, 6] and eng.calls[-1]["F"] == 6
    each = rovmpc.calibrate_cable(np.zeros(3), P1b, Yb, guess=gb, arc=arc, groups="each", free_length=False, L0=2.7, engine=eng)
    assert each.L.shape == (6,) and list(eng.calls[-1]["off"]) == list(range(7)) and (each.L == 2.7).all() and np.isnan(each.sigma_L).all()
    offs = rovmpc.calibrate_cable(np.zeros(3), P1b, Yb, guess=gb, arc=arc, groups=[0, 2, 2, 6], engine=eng)
    assert offs.L.shape == (3,) and offs.status[1] == rovmpc.CalibStatus.NO_FRAMES and offs.n_active.tolist() == [2, 0, 4]
    # a CableTrack as the guess: its angles
    track = rovmpc.CableTrack(*([r["guess"][:, 0], r["guess"][:, 1]] + [np.zeros(6)] * 7 + [np.zeros(2)]))
    rovmpc.calibrate_cable(r["P0"], r["P1"], r["Y"], guess=track, arc=arc, engine=eng)
    assert np.array_equal(eng.calls[-1]["guess"], r["guess"]) and eng.calls[-1]["guess"].shape == (6, 2)
    n = len(eng.calls)
    for kw in (dict(groups="all"), dict(groups=[0, 3]), dict(groups=[1, 6]), dict(groups=[0, 4, 3, 6]), dict(groups=[0.0, 6.0]),
               dict(arc=arc[::-1]), dict(arc=arc[:5]), dict(arc=np.where(np.arange(16) == 4, np.nan, arc))):
        with pytest.raises(ValueError):
            rovmpc.calibrate_cable(**{**dict(P0=r["P0"], P1=r["P1"], markers=r["Y"], guess=r["guess"], arc=arc, engine=eng), **kw})
    for Y in (r["Y"][0], r["Y"][:, :2], np.zeros((2, 3, 4, 5, 3))):
        with pytest.raises(ValueError):
            rovmpc.calibrate_cable(r["P0"][0], r["P1"][0], Y, engine=eng)
    assert len(eng.calls) == n                                              # refused before the engine was reached


def test_config_of_a_calibration():
    eng = StandInEngine()
    r = cf.recording(4, 2.7, seed=3)
    cal = rovmpc.calibrate_cable(r["P0"], r["P1"], r["Y"], guess=r["guess"], arc=r["arc"], engine=eng)
    cfg = rovmpc.MPCConfig(N=7)
    new = cal.config(cfg)
    assert new.L == float(cal.L) and new.N == 7 and cfg.L == 3.0 and new == dataclasses.replace(cfg, L=float(cal.L))
    cut = rovmpc.calibrate_cable(r["P0"], r["P1"], r["Y"], guess=r["guess"], arc=r["arc"], max_iter=1, engine=eng)
    with pytest.raises(ValueError, match="MAX_ITER"):
        cut.config(cfg)
    two = rovmpc.calibrate_cable(r["P0"], r["P1"], r["Y"], guess=r["guess"], arc=r["arc"], groups=[0, 2, 4], engine=eng)
    with pytest.raises(ValueError, match="exactly one group"):
        two.config(cfg)


def test_header_and_struct_mirror_agree():
    hdr = open(os.path.join(cf.ROOT, "include", "rovmpc.h")).read()
    body = re.search(r"typedef struct rovmpc_calib_params \{(.*?)\} rovmpc_calib_params;", hdr, re.S).group(1)
    names = [n for decl in re.findall(r"^\s*(?:int32_t|double)\s+([^;]+);", body, re.M) for n in re.split(r"\s*,\s*", decl)]
    assert names == [n for n, _ in rovmpc.CalibParams._fields_]
    assert C.sizeof(rovmpc.CalibParams) == 56
    for name, val in (("ROVMPC_CALIB_GROUP_OUT", 8), ("ROVMPC_CALIB_FRAME_OUT", 5), ("ROVMPC_CALIB_STALLED", 6), ("ROVMPC_CALIB_NO_FRAMES", 7)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    assert [s.value for s in rovmpc.CalibStatus] == list(range(8)) and rovmpc.CalibStatus.STALLED == cf.STALLED
    p = rovmpc.CalibParams.make()
    assert (p.max_iter, p.free_length, p.L_lo, p.tol, p.tol_L) == (60, 1, 0.0, 1e-12, 1e-12) and np.isnan(p.L0) and p.L_hi == float("inf")
    for kw in (dict(max_iter=0), dict(max_iter=2.5), dict(tol=-1), dict(tol_L=float("nan")), dict(L0=0), dict(L0=float("inf")), dict(L_lo=2, L_hi=2)):
        with pytest.raises(ValueError):
            rovmpc.CalibParams.make(**kw)
