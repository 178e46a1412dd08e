"""The cable-length calibration on the GPU (rovmpc_calibrate_cable, rovmpc_calibrate_cable_device, rovmpc_cable_markers; law
in include/rovmpc.h): the forward model against 50 digits, the tie to rovmpc_fit_theta_gamma bit for bit, the recovery of L
from arc-placed markers, the noisy minimiser, what the index rule does to such markers, planted frames, the bits'
independence of the grouping and the entry, and the refused arguments.  Allowances: tests/golden/calib_bounds.json, measured
on the NumPy restatement by tests/test_calib_reference_host.py; the GPU gets 4 x those."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_reference as cf  # noqa: E402
import fit_reference as fr  # noqa: E402
from plan_controller_helpers import rv  # noqa: E402,F401
from plan_loop_helpers import same  # noqa: E402

pytestmark = pytest.mark.gpu

GPU_FACTOR = 4.0


def engine(rv, up=1.0, L=cf.L_WS):
    return rv.Engine(rv.MPCConfig(N=1, K=1, dtype="f64", c_lo=cf.BRACKET[0], c_hi=cf.BRACKET[1], L=L, frame="ENU" if up > 0 else "NED"))


@pytest.fixture(scope="module")
def eng(rv):
    with engine(rv) as e:
        yield e


def forward_of(e):
    return lambda P0, P1, th, ga, L, arc, M: e.cable_markers(P0, P1, th, ga, L=np.full(len(th), L), arc=arc, M=M)


# ---- 1. the forward model ----------------------------------------------------------------------------------------------------

def test_forward_model_against_50_digits(eng):
    from mpmath import mp
    bound = GPU_FACTOR * cf.bounds()["forward_np_max_err_uL"]
    worst = 0.0
    for M in cf.FORWARD_M:
        for arc in (cf.uniform_arc(M), cf.uneven_arc(M)):
            for name, A, P, th, ga, L in cf.forward_cases():
                X = eng.cable_markers(A, P, th, ga, L=L, arc=arc, M=M)
                assert X.shape == (M, 3)
                if name == "nan-angle":
                    assert np.isnan(X).all()
                    continue
                ref, chord = cf.markers_mp(A, P, th, ga, L, arc, M)
                assert chord == (name == "chord")
                with mp.workdps(cf.DPS):
                    err = max(float(abs(cf._mp(X[m, i]) - ref[m][i])) for m in range(M) for i in range(3)) / (cf.EPS * L)
                worst = max(worst, err)
                assert same(X[0], np.asarray(A, float) + 0.0) and np.abs(X[-1] - P).max() <= 4 * cf.EPS * L, name
                assert err <= bound, (name, M, err, bound)
    print(f"forward model: largest error {worst:.3g} u L (allowed {bound:.3g})")


def test_asinh_through_the_placement(rv):
    """m_asinh through the entry: the level cables of calib_reference.asinh_cases take its argument from 2^-60 to e^16; the error in units of
    u L (1 + kappa'), kappa' the conditioning of the cable's root, which every point inherits."""
    from mpmath import mp
    bound = GPU_FACTOR * cf.bounds()["asinh_np_max_err_uL"]
    worst, lo, hi = 0.0, np.inf, 0.0
    M = len(cf.ASINH_ARC)
    for case in cf.asinh_cases():
        A, P, th, ga, L, bracket, _ = case
        with rv.Engine(rv.MPCConfig(N=1, K=1, dtype="f64", c_lo=bracket[0], c_hi=bracket[1], L=3.0)) as e:
            X = e.cable_markers(A, P, th, ga, L=L, arc=cf.ASINH_ARC, M=M)
        ref, chord = cf.markers_mp(A, P, th, ga, L, cf.ASINH_ARC, M, bracket=bracket)
        assert not chord and np.isfinite(X).all()
        xs, kappa = cf.asinh_arguments(case)
        lo, hi = min(lo, min(x for x in xs if x > 0)), max(hi, max(xs))
        with mp.workdps(cf.DPS):
            err = max(float(abs(cf._mp(X[m, i]) - ref[m][i])) for m in range(M) for i in range(3)) / (cf.EPS * L * (1.0 + kappa))
        worst = max(worst, err)
        assert err <= bound, (P, err, bound)
    print(f"asinh through the placement: |x| from {lo:.3g} to {hi:.3g}, largest error {worst:.3g} u L (1 + kappa') (allowed {bound:.3g})")
    assert lo <= 2.0 ** -60 and hi >= math.exp(16), (lo, hi)


def test_index_rule_is_the_fits_model_bit_for_bit(rv):
    """arc = NULL, L = NULL: the points are the fit's model's.  The fit's kernel exposes its model only through its residual
    r = (X - A) - (Y - A), so the forward model's points are fed back as markers at the same angles: rms0 must be +0 to the bit
    (F = sum |X - Y|^2 with X the same bits), at M = 3, 5 and 16, ENU and NED.  A = 0 throughout: with another anchor the
    fit's own (Y - A) rounds, and the check would no longer be exact."""
    n = 0
    for up in (1.0, -1.0):
        for M in (3, 5, 16):
            fs = [f for f in fr.scenes() if f.truth is not None and not f.noisy and not np.any(f.A) and np.isfinite(f.Y).all()]
            fs = [f for f in fs if f.up == 1.0 and f.M == 16][:6]               # geometries; the frame is mirrored for NED below
            A = np.zeros((len(fs), 3))
            P = np.array([f.P * [1.0, 1.0, up] for f in fs])
            th, ga = np.array([f.truth[0] for f in fs]), np.array([f.truth[1] for f in fs])
            with engine(rv, up) as e:
                X = e.cable_markers(A, P, th, ga, M=M)
                fit = e.fit_theta_gamma(A, P, X, guess=np.stack([th, ga], axis=1), max_iter=1)
            assert X.shape == (len(fs), M, 3) and np.isfinite(X).all()
            assert same(np.asarray(fit.rms0, dtype=np.float64), np.zeros(len(fs))), (up, M, fit.rms0)
            assert (np.abs(X[:, M // 2] - 0.5 * P).max(axis=1) > 1e-3).all()     # catenaries, not chords
            n += len(fs)
    assert n == 36


# ---- 2. the tie ------------------------------------------------------------------------------------------------------------------

def test_one_frame_groups_with_a_fixed_length_are_the_fit_bit_for_bit(rv):
    by = {}
    for i, f in enumerate(fr.scenes()):
        by.setdefault((f.up, f.M, f.max_iter), []).append(i)
    seen = set()
    for (up, M, max_iter), idx in by.items():
        fs = [fr.scenes()[i] for i in idx]
        A, P, Y = np.array([f.A for f in fs]), np.array([f.P for f in fs]), np.array([f.Y for f in fs])
        guess = np.array([(0.0, 0.0) if f.guess is None else f.guess for f in fs])
        with engine(rv, up) as e:
            fit = e.fit_theta_gamma(A, P, Y, guess=guess, max_iter=max_iter)
            og, of = e.calibrate_cable(A, P, Y, np.arange(len(fs) + 1), guess=guess, free_length=False, max_iter=max_iter)
        for k, f in enumerate(fs):
            want = np.array([fit.theta[k], fit.gamma[k], fit.rms[k], fit.rms0[k], float(fit.status[k]), float(fit.iters[k])])
            got = np.array(list(of[k]) + [og[k, 4]])
            assert same(got, want), (f.name, got, want)
            seen.add(int(fit.status[k]))
            assert og[k, 5] == (fit.status[k] if fit.status[k] < 2 or fit.iters[k] > 0 else cf.NO_FRAMES), (f.name, og[k])
    assert seen == {0, 1, 2, 3, 4, 5}, seen


# ---- 3. recovery ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def recovery(eng):
    """Per (L_true, frames, M): the recording (markers from the engine's own forward model), the restatement's and the GPU's
    outputs, all groups of one L_true in ONE call."""
    out = {}
    for L_true in (2.7, 3.3):
        recs = [cf.recording(n, L_true, seed=n + M, M=M, forward=forward_of(eng)) for n, M in cf.RECOVERY_GROUPS]
        for (n, M), r in zip(cf.RECOVERY_GROUPS, recs):
            ref = cf.calib_np(r["P0"], r["P1"], r["Y"], r["guess"], r["arc"], L0=3.0)
            og, of = eng.calibrate_cable(r["P0"], r["P1"], r["Y"], [0, n], guess=r["guess"], arc=r["arc"])
            out[(L_true, n, M)] = (r, ref, og[0], of)
    return out


def test_recovery_of_the_length_from_arc_placed_markers(recovery):
    b = cf.bounds()
    for (L_true, n, M), (r, ref, og, of) in recovery.items():
        assert ref.group[5] == cf.CONVERGED and 4 <= ref.group[4] <= 8, (L_true, n, M, ref.group)           # the input is known good
        assert og[5] == cf.CONVERGED and og[4] == ref.group[4] and og[6] == n and og[7] == n * M, (L_true, n, M, og)
        eL = abs(og[0] - L_true)
        ea = max(np.abs(of[:, 0] - r["theta"]).max(), np.abs(of[:, 1] - r["gamma"]).max())
        print(f"L = {L_true} frames {n:3d} M {M:2d}: trial steps {int(og[4])}, |dL| {eL:.3g}, angle error {ea:.3g}, rms {og[1]:.3g}")
        assert eL <= GPU_FACTOR * b["recovery_np_max_err_L"] and ea <= GPU_FACTOR * b["recovery_np_max_err_angle"]
        assert (of[:, 4] == cf.CONVERGED).all() and og[1] <= 1e-13


# ---- 4. the noisy minimiser -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def noisy():
    return cf.recording(**cf.NOISY)


def test_noisy_recording_lands_on_the_50_digit_minimiser(eng, noisy):
    from mpmath import mp, mpf
    r = noisy
    with open(os.path.join(cf.GOLDEN, "calib_minimisers.json")) as f:
        gold = json.load(f)
    b = cf.bounds()
    og, of = eng.calibrate_cable(r["P0"], r["P1"], r["Y"], [0, len(r["Y"])], guess=r["guess"], arc=r["arc"], tol=cf.NOISY_TOL, tol_L=cf.NOISY_TOL)
    og = og[0]
    assert og[5] == cf.CONVERGED and og[6] == cf.NOISY["n"], og
    with mp.workdps(cf.DPS):
        dL = float(abs(cf._mp(og[0]) - mpf(gold["L"])))
        da = max(max(float(abs(cf._mp(of[f, 0]) - mpf(gold["theta"][f]))), float(abs(cf._mp(of[f, 1]) - mpf(gold["gamma"][f]))))
                 for f in range(len(of)))
    print(f"noisy: L^ {og[0]:.12f} sigma_L {og[3]:.3g} trial steps {int(og[4])}; to the minimiser: L {dL:.3g} angle {da:.3g} "
          f"(NumPy {b['noisy_np_distance_L']:.3g}, {b['noisy_np_distance_angle']:.3g}); |L^ - L_true| / sigma_L {abs(og[0] - 2.7) / og[3]:.3g}")
    assert dL <= GPU_FACTOR * b["noisy_np_distance_L"] and da <= GPU_FACTOR * b["noisy_np_distance_angle"]
    assert abs(og[0] - cf.NOISY["L_true"]) <= 3.0 * og[3]


# ---- 5. why: the index rule on arc-placed markers ----------------------------------------------------------------------------------

def test_index_rule_on_arc_placed_markers_misses_the_length(recovery, eng):
    r = recovery[(2.7, 128, 16)][0]
    og, _ = eng.calibrate_cable(r["P0"], r["P1"], r["Y"], [0, 128], guess=r["guess"], arc=None)
    print(f"index rule on arc-placed markers: L^ {og[0, 0]:.4f}, status {int(og[0, 5])}, rms {og[0, 1]:.3g}")
    assert og[0, 5] != cf.CONVERGED or abs(og[0, 0] - 2.7) > 0.1


# ---- 6. planted frames -----------------------------------------------------------------------------------------------------------

def planted(eng):
    r = cf.recording(20, 2.7, seed=99, forward=forward_of(eng))
    P0, P1, Y, guess = r["P0"].copy(), r["P1"].copy(), r["Y"].copy(), r["guess"].copy()
    P1[3, 1] = np.nan                                                       # NONFINITE
    Y[7, 1:-1] = np.nan                                                     # TOO_FEW
    P1[11] = [2.5, 1.5, 1.2]                                                # CHORD: 3.15 m, longer than L0 = 3
    P1[15] = [0.0, 0.0, 1.5]; guess[15] = 0.0                               # DEGENERATE: a vertical chord at theta = 0
    cls = {3: cf.NONFINITE, 7: cf.TOO_FEW, 11: cf.CHORD, 15: cf.DEGENERATE}
    return r, P0, P1, Y, guess, cls


def test_planted_frames_are_left_out_exactly(eng):
    r, P0, P1, Y, guess, cls = planted(eng)
    og, of = eng.calibrate_cable(P0, P1, Y, [0, 20], guess=guess, arc=r["arc"])
    keep = np.array([f not in cls for f in range(20)])
    og2, of2 = eng.calibrate_cable(P0[keep], P1[keep], Y[keep], [0, 16], guess=guess[keep], arc=r["arc"])
    assert og[0, 5] == cf.CONVERGED and og[0, 6] == 16 and same(og[0], og2[0]) and same(of[keep], of2)
    bad = np.array(sorted(cls))
    fit = eng.fit_theta_gamma(P0[bad], P1[bad], Y[bad], guess=guess[bad])
    for k, f in enumerate(bad):
        assert of[f, 4] == cls[f] == fit.status[k], (f, of[f], fit.status[k])
        if cls[f] in (cf.NONFINITE,):
            assert np.isnan(of[f, :4]).all()
        elif cls[f] == cf.TOO_FEW:              # the fit's outputs at L0: the same bits (the end markers alone: index rule = arc rule)
            assert same(of[f, :4], np.array([fit.theta[k], fit.gamma[k], fit.rms[k], fit.rms0[k]]))
        else:
            assert same(of[f, :2], guess[f]) and of[f, 2] == of[f, 3]
    # only such frames; one trial step; the box
    og3, of3 = eng.calibrate_cable(P0[bad], P1[bad], Y[bad], [0, 4], guess=guess[bad], arc=r["arc"])
    assert og3[0, 5] == cf.NO_FRAMES and og3[0, 6] == 0 and og3[0, 0] == 3.0 and og3[0, 4] == 0 and (of3[:, 4] == [cls[f] for f in bad]).all()
    og4, _ = eng.calibrate_cable(P0[keep], P1[keep], Y[keep], [0, 16], guess=guess[keep], arc=r["arc"], max_iter=1)
    assert og4[0, 5] == cf.MAX_ITER_S and og4[0, 4] == 1
    og5, _ = eng.calibrate_cable(r["P0"][keep], r["P1"][keep], r["Y"][keep], [0, 16], guess=guess[keep], arc=r["arc"], L0=2.5, L_hi=2.69,
                                 max_iter=30)
    print(f"box (0, 2.69) around a 2.7 m cable: L^ {og5[0, 0]:.6f}, status {int(og5[0, 5])}, trial steps {int(og5[0, 4])}")
    assert 0 < og5[0, 0] < 2.69


# ---- 7. independence, to the bit ---------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_grouping_order_or_entry(rv, eng, recovery):
    keys = [(2.7, 1, 16), (2.7, 2, 16), (2.7, 129, 16), (3.3, 128, 16)]
    recs = [recovery[k] for k in keys]
    cat = lambda name, order: np.concatenate([recs[i][0][name] for i in order])
    arc = recs[0][0]["arc"]

    def run(order, **kw):
        off = np.concatenate([[0], np.cumsum([len(recs[i][0]["Y"]) for i in order])])
        return eng.calibrate_cable(cat("P0", order), cat("P1", order), cat("Y", order), off, guess=cat("guess", order), arc=arc, **kw), off

    (og, of), off = run([0, 1, 2, 3])
    for i in range(4):                                                       # alone (the recovery fixture's calls) against among the others
        assert same(og[i], recs[i][2]) and same(of[off[i]:off[i + 1]], recs[i][3]), keys[i]
    (ogp, ofp), offp = run([2, 0, 3, 1])
    for j, i in enumerate([2, 0, 3, 1]):
        assert same(ogp[j], og[i]) and same(ofp[offp[j]:offp[j + 1]], of[off[i]:off[i + 1]])
    (ogd, ofd), _ = run([0, 1, 2, 3], device=True)                           # host against device entry
    assert same(ogd, og) and same(ofd, of)
    (og2, of2), _ = run([0, 1, 2, 3])                                        # again on the same handle: buffers reused, done words reset
    assert same(og2, og) and same(of2, of)
    r = recs[2][0]                                                           # "pooled" against explicit offsets, through the public call
    a = rv.calibrate_cable(r["P0"], r["P1"], r["Y"], guess=r["guess"], arc=arc, engine=eng)
    b = rv.calibrate_cable(r["P0"], r["P1"], r["Y"], guess=r["guess"], arc=arc, groups=np.array([0, 129]), engine=eng)
    assert same(np.float64(a.L), b.L[0]) and same(a.theta, b.theta) and same(np.float64(a.L), recs[2][2][0])
    assert a.config(rv.MPCConfig()).L == a.L


# ---- 8. arguments ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_launch_nothing_and_leave_the_outputs(rv, eng):
    r = cf.recording(4, 2.7, seed=5)
    lib, h = eng.lib, eng._h
    P0, P1, Y = (np.ascontiguousarray(r[k]) for k in ("P0", "P1", "Y"))
    off, arc = np.array([0, 4], np.int32), np.ascontiguousarray(r["arc"])
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    P = rv.CalibParams

    def call(P0=P0, P1=P1, Y=Y, F=4, M=16, off=off, G=1, arc=arc, params=None, og="out", of="out"):
        g, f = np.full((1, 8), 7.0), np.full((4, 5), 7.0)
        rc = lib.rovmpc_calibrate_cable(h, p(P0), p(P1), p(Y), F, M, p(off), G, None, p(arc), None if params is None else C.byref(params),
                                        p(g) if og == "out" else None, p(f) if of == "out" else None)
        return rc, g, f

    def params(**kw):
        q = P.make()
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    rc, g, f = call()
    assert rc == 0 and g[0, 5] == cf.CONVERGED
    bad_arc = [arc[::-1].copy(), np.where(np.arange(16) == 5, arc[4], arc), np.where(np.arange(16) == 0, 0.01, arc),
               np.where(np.arange(16) == 15, 0.99, arc), np.where(np.arange(16) == 3, np.nan, arc)]
    bad = [dict(P0=None), dict(Y=None), dict(off=None), dict(og=None), dict(of=None), dict(M=2), dict(M=17), dict(F=-1), dict(G=-1),
           dict(off=np.array([1, 4], np.int32)), dict(off=np.array([0, 3], np.int32)), dict(off=np.array([0, 3, 2, 4], np.int32), G=3)]
    bad += [dict(arc=a) for a in bad_arc]
    bad += [dict(params=params(**kw)) for kw in (dict(struct_size=8), dict(max_iter=0), dict(max_iter=1001), dict(L0=0.0), dict(L0=-1.0),
                                                   dict(L0=float("inf")), dict(L_lo=3.0, L_hi=3.0), dict(L_lo=float("nan")), dict(L_lo=3.5),
                                                   dict(tol=-1.0), dict(tol=float("nan")), dict(tol_L=-1e-3), dict(tol_L=float("nan")))]
    for kw in bad:
        rc, g, f = call(**kw)
        assert rc == -1, (kw, rc)                                            # ROVMPC_ERR_INVALID
        assert (g == 7.0).all() and (f == 7.0).all() and eng.lib.rovmpc_last_error(h), kw
    assert call(F=0, off=np.array([0, 0], np.int32))[0] == 0 and call(G=0)[0] == 0
    out = np.full((2, 16, 3), 7.0)
    th = np.zeros(2)
    for kw in (dict(M=2), dict(arc=bad_arc[0]), dict(th=None)):
        rc = lib.rovmpc_cable_markers(h, p(P0), p(P1), p(kw.get("th", th)), p(th), None, p(kw.get("arc", arc)), 2, kw.get("M", 16), p(out))
        assert rc == -1 and (out == 7.0).all(), kw
    assert lib.rovmpc_cable_markers(h, None, None, None, None, None, None, 0, 16, None) == 0
