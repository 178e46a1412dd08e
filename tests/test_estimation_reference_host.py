"""CPU check of the 50-digit estimation references (tests/estimation_reference.py) and of the margins the GPU tests use.

Each margin m is fixed from the float64 oracle's largest error / bound ratio at m = 1 over the whole workspace, and the ratio it
was fixed from stands next to it: m_R = 4 x ratio rounded up (LAPACK's bidiagonalisation and the kernel's one-sided Jacobi are
two float64 algorithms with a backward error each, and a factor 2 is left for the order of the sums), every other m = 2 x ratio
rounded up (the same sums in another order).  The tests re-measure the ratios, print them and hold the oracle to m / 4 (m / 2)."""
import math
import os

import numpy as np
import pytest

import estimation_reference as er

# margin, and the oracle's measured largest ratio it comes from
M_R, RATIO_R = 15, 3.7188                  # |R - R*|, |v_out - R* v| of Kabsch (numpy.linalg.svd)
M_GAUSS, RATIO_GAUSS = 2, 0.7229          # scipy.ndimage.gaussian_filter1d
M_SAVGOL, RATIO_SAVGOL = 2, 0.7920        # numpy's product of the host-built hat-matrix rows (not scipy's savgol_filter: see its test)
M_GRAD, RATIO_GRAD = 2, 0.6296            # numpy.gradient
M_SWAY, RATIO_SWAY = 2, 0.7707           # v_sway, v_surge of the oracle's features_dd
M_FEAT, RATIO_FEAT = 2, 0.9889           # unit vector, clipped length and clipped cosine of the oracle's feature map
DEFECT_ORACLE = 2.0e-15                   # largest |R R^T - I|_max of the oracle over the decided frames
DEFECT_BOUND = 4 * DEFECT_ORACLE        # what the kernel's R (decided or not) has to meet


@pytest.fixture(scope="module")
def orc():
    from oracle import rovmpc_oracle
    return rovmpc_oracle


def _fixed(m, ratio_recorded, ratio, factor, what):
    print("%s: oracle's largest ratio %.4f (recorded %.4f), m = %d x ratio rounded up = %d (recorded %d)"
          % (what, ratio, ratio_recorded, factor, math.ceil(factor * ratio), m))
    assert ratio <= m / factor, what
    assert m == math.ceil(factor * ratio_recorded)


def test_kabsch_workspace_families():
    for M in er.MS:
        fr = er.kabsch_workspace(M)
        assert len(fr) % 128 == 1 and len(fr) >= 257
        assert {f.family for f in fr} == set("abcdefg")
        assert all(f.P.shape == (M, 3) and f.Q.shape == (M, 3) for f in fr)
        again = er.kabsch_workspace.__wrapped__(M)
        assert all(np.array_equal(f.P, g.P) and np.array_equal(f.Q, g.Q) and np.array_equal(f.v, g.v) for f, g in zip(fr, again))
        t = er.kabsch_table(M)
        fam = lambda x: np.array([f.family == x for f in fr])
        tag = lambda x: np.array([f.tag == x for f in fr])
        # what each family is for
        ang = [float(f.tag[6:]) for f in fr if f.tag.startswith("angle=")]
        assert min(ang) == 0.0 and max(ang) == pytest.approx(math.pi, abs=1e-4)
        if M > 3:                                # three markers span a plane: sigma_3 = 0 and d is a matter of convention
            assert (t.d[fam("d")] == -1).all()
            r32 = t.sigma[:, 2] / t.sigma[:, 1]
            for name, want in (("0.5", 0.5), ("1e-3", 1e-3), ("1e-6", 1e-6)):
                assert r32[tag(name) & fam("d")] == pytest.approx(want, rel=1e-3)
            assert 1 - r32[tag("sigma2~sigma3")] == pytest.approx(1e-6, rel=1e-2)
        eq = fam("e") & np.array(["noise" not in f.tag for f in fr])
        assert (np.abs(t.sigma[eq, 1] / t.sigma[eq, 0] - 1) < 1e-12).all()
        assert any(np.array_equal(f.P, f.Q) for f in fr)
        assert {f.tag for f in fr if f.family == "g"} == {"k=%+d" % (s * k) for k in (10, 100, 400) for s in (1, -1)}
        assert np.abs(t.P[tag("k=+400")]).max() > 2.0 ** 398 and np.abs(t.P[tag("k=-400")]).max() < 2.0 ** -396
        assert np.abs(t.P[fam("b")]).max() > 5e3
        # the exclusion cap: only near-collinear frames and the one sigma_2 ~ sigma_3 frame may be undecided
        und = ~t.decided
        assert (fam("f") | tag("sigma2~sigma3"))[und].all(), [fr[i].tag for i in np.nonzero(und)[0]]
        assert und[fam("f") & np.array([f.tag.startswith("collinear") or f.tag in ("1e-9", "1e-12") for f in fr])].all()
        col = np.array([f.tag.startswith("collinear") for f in fr])
        assert col.sum() == 50 and (t.sigma[col, 1] < 1e-10 * t.sigma[col, 0]).all()
        assert t.decided[tag("1e-3")].all()
        print("M = %d: %d frames, undecided: %s" % (M, len(fr), sorted({(fr[i].family, fr[i].tag.split(",")[0]) for i in np.nonzero(und)[0]})))


def test_kabsch_reference_is_a_rotation_that_solves_the_problem():
    """R* is orthogonal with det +1 to 1e-45, and no nearby rotation fits the centred sets better."""
    from mpmath import mp, mpf
    fr = er.kabsch_workspace(4)
    for f in fr[::16]:
        tr = er.kabsch_true(f.P, f.Q, f.v)
        with mp.workdps(er.DPS):
            assert mp.norm(tr.R * tr.R.T - mp.eye(3), mp.inf) < mpf("1e-45") and abs(mp.det(tr.R) - 1) < mpf("1e-45")
        R = np.array(tr.R.tolist(), float)
        Pc, Qc = f.P - f.P.mean(axis=0), f.Q - f.Q.mean(axis=0)
        scale = max(np.abs(Pc).max() * np.abs(Qc).max(), 1e-300)
        fit = lambda X: np.trace(X @ (Pc.T @ Qc) / scale)          # Kabsch maximises tr(R H)
        for ax in np.eye(3):
            for s in (1e-4, -1e-4):
                assert fit(er.rotation(ax, s) @ R) <= fit(R) * (1 + 1e-12) + 1e-12


def test_kabsch_margin_of_the_plain_reference(orc):
    worst_R = worst_v = defect = 0.0
    for M in er.MS:
        t = er.kabsch_table(M)
        R = np.empty((len(t.frames), 3, 3))
        with np.errstate(all="ignore"):
            for i, f in enumerate(t.frames):
                R[i] = orc.compute_rotation_kabsch(f.P, f.Q)
        v = np.einsum("tij,tj->ti", R, t.v)
        eR, ev = er.kabsch_errors(t, R, v)
        bR, bv = er.kabsch_bounds(t, 1.0)
        dec = t.decided
        worst_R = max(worst_R, float((eR[dec] / bR[dec]).max()))
        # the v bound's 4 eps are the product's own roundings: the ratio is that of the R part alone
        worst_v = max(worst_v, float(((ev[dec] - 4 * er.EPS * np.abs(t.v[dec]).sum(axis=1)) / (bR[dec] * np.abs(t.v[dec]).sum(axis=1))).max()))
        defect = max(defect, float(er.orthogonality_defect(R[dec]).max()))
        assert (np.linalg.det(R[dec]) > 0).all()
    print("Kabsch, oracle: largest ratio R %.4f, v_out (R part) %.4f, orthogonality defect %.3g (recorded %.3g)" % (worst_R, worst_v, defect, DEFECT_ORACLE))
    _fixed(M_R, RATIO_R, worst_R, 4, "m_R")
    assert worst_v <= M_R / 4
    assert defect <= DEFECT_ORACLE and DEFECT_ORACLE <= 2 * defect and DEFECT_BOUND == 4 * DEFECT_ORACLE


def test_gaussian_margin_of_the_plain_reference():
    from scipy.ndimage import gaussian_filter1d
    worst = 0.0
    for T, sigma in er.GAUSS_CASES:
        x = er.signal(T, 100 + T)
        ref = er.gaussian_reference(x, sigma)
        worst = max(worst, float((er.err(gaussian_filter1d(x, sigma), ref.hi, ref.lo) / ref.scale).max()))
    _fixed(M_GAUSS, RATIO_GAUSS, worst, 2, "m_gauss")
    w = er.gaussian_weights(3.5)
    assert len(w) == 15 and abs(w[0] + 2 * sum(w[1:]) - 1) < 4 * er.EPS
    assert [er.reflect(j, 6) for j in (-1, -6, -7, -12, -13, 6, 11, 12, 19)] == [0, 5, 5, 0, 0, 5, 0, 0, 4]


def _savgol_numpy(x, window, order):
    W, half, T = er.savgol_hat(window, order), window // 2, len(x)
    y = np.empty(T)
    for i in range(T):
        first = 0 if i < half else T - window if i >= T - half else i - half
        y[i] = np.dot(W[i - first if (i < half or i >= T - half) else half], x[first:first + window])
    return y


def test_savgol_margin_of_the_plain_reference():
    """The oracle of these sums is numpy's float64 product of the same hat-matrix rows.  scipy.signal.savgol_filter is not:
    it fits the edge polynomials by least squares anew (polyfit / polyval), which costs it three decimal digits; its ratio is
    printed for the record and bounded by the tolerance the existing parity test grants it."""
    from scipy.signal import savgol_filter
    worst = worst_scipy = 0.0
    for T, window, order in er.SAVGOL_CASES:
        x = er.signal(T, 200 + T + window)
        ref = er.savgol_reference(x, window, order)
        worst = max(worst, float((er.err(_savgol_numpy(x, window, order), ref.hi, ref.lo) / ref.scale).max()))
        e = er.err(savgol_filter(x, window, order), ref.hi, ref.lo)
        worst_scipy = max(worst_scipy, float((e / ref.scale).max()))
        assert (e <= 1e-9 * np.abs(ref.hi) + 1e-12).all()
    print("scipy.signal.savgol_filter against the same bound: largest ratio %.1f" % worst_scipy)
    _fixed(M_SAVGOL, RATIO_SAVGOL, worst, 2, "m_savgol")
    for window, order in ((11, 3), (21, 5)):
        H, X = er.savgol_hat(window, order), er.savgol_hat_exact(window, order)
        assert np.abs(H - X).max() <= 2 * er.EPS * np.abs(X).max()        # the host's construction is the exact projector, rounded


def test_gradient_margin_of_the_plain_reference():
    worst = 0.0
    for T in er.GRAD_TS:
        for kind in ("uniform", "jitter"):
            t = er.times(T, kind, 300 + T)
            if kind == "jitter" and T > 3:
                dt = np.diff(t)
                assert (dt[1:] / dt[:-1]).max() == pytest.approx(100.0, rel=1e-6) and (dt[1:] / dt[:-1]).min() < 0.02
            f = er.signal(T, 400 + T)
            g = er.gradient_reference(f, t)
            worst = max(worst, float((er.err(np.gradient(f, t), g.ref.hi, g.ref.lo) / g.ref.scale).max()))
    _fixed(M_GRAD, RATIO_GRAD, worst, 2, "m_grad")


def test_chained_gradients_of_the_plain_reference():
    """The float64 chain (hat-matrix rows, np.gradient, np.gradient) stays within the bounds carried with m / 2."""
    worst = [0.0, 0.0, 0.0]
    for T in (11, 256, 257):
        for kind in ("uniform", "jitter"):
            t = er.times(T, kind, 300 + T); x = er.signal(T, 600 + T)
            ch = er.derivative_chain(x, t)
            y0 = _savgol_numpy(x, 11, 3); y1 = np.gradient(y0, t); y2 = np.gradient(y1, t)
            b = er.chain_bounds(ch, M_SAVGOL / 2, M_GRAD / 2)
            for k, (got, ref) in enumerate(((y0, ch.smooth), (y1, ch.d1.ref), (y2, ch.d2.ref))):
                e = er.err(got, ref.hi, ref.lo)
                worst[k] = max(worst[k], float((e / b[k]).max()))
                assert (e <= b[k]).all(), (T, kind, k)
    print("oracle's chain against half the carried bounds: smooth %.3f, first gradient %.3f, second gradient %.3f" % tuple(worst))


def test_feature_map_margin_of_the_plain_reference(orc):
    worst = worst_g = 0.0
    for T in er.FEATURE_TS:
        P0, P1, V1, t, th, ga = er.feature_inputs(T)
        rel = P1 - P0
        nr = np.linalg.norm(rel, axis=1)
        if T > 250:          # the rows the map's guards and clips are for
            assert (nr == 0).any() and (nr > 10).any() and ((nr > 0) & (nr < 1e-5)).any() and (np.abs(V1).sum(axis=1) == 0).any()
        ref = er.features_reference(P0, P1, V1, t, th, ga)
        with np.errstate(all="ignore"):
            X = orc.extract_features_gen1(P0, P1, V1, t, th, ga)
        assert np.array_equal(X[:, er.EXACT_COLS], ref.hi[:, er.EXACT_COLS])
        e = er.err(X, ref.hi, ref.lo)
        cols = [9, 10, 11, 12, 13]
        ok = ref.scale[:, cols] > 0
        assert (e[:, cols][~ok] == 0).all()
        worst = max(worst, float((e[:, cols][ok] / ref.scale[:, cols][ok]).max()))
        okg = ref.scale[:, 6:9] > 0
        worst_g = max(worst_g, float((e[:, 6:9][okg] / ref.scale[:, 6:9][okg]).max()))
        assert (e[:, 6:9][~okg] == 0).all()
        assert (np.abs(X[:, 13]) <= 1).all() and X[:, 12].min() >= 1e-5 and X[:, 12].max() <= 10.0
        if T > 250:
            u = rel / (nr + 1e-8)[:, None]
            raw = np.sum(V1 * u, axis=1) / (np.linalg.norm(V1, axis=1) + 1e-8)
            assert raw.max() > 1.0 and raw.min() < -1.0                  # the clip of the cosine has something to do
            assert X[:, 13].max() == 1.0 and X[:, 13].min() == -1.0 and X[:, 12].min() == 1e-5 and X[:, 12].max() == 10.0
    print("feature map, oracle: gradient columns' largest ratio %.4f of m_grad / 2 = %g" % (worst_g, M_GRAD / 2))
    assert worst_g <= M_GRAD / 2
    _fixed(M_FEAT, RATIO_FEAT, worst, 2, "m_feat")


def test_surge_sway_margin_of_the_plain_reference(orc):
    worst = 0.0
    for T in (11, 257):
        rng = np.random.default_rng(800 + T + 11)
        P0 = rng.normal(size=(T, 3)) * 300 + rng.uniform(-1e4, 1e4, size=3)
        P1 = P0 + rng.normal(size=(T, 3)) * 900
        V = rng.normal(size=(T, 3)) * 200
        sway, surge = er.surge_sway_reference(P0, P1, V)
        got_sway, got_surge = orc._dd_surge_sway(P0 / 1000, P1 / 1000, V / 1000)
        worst = max(worst, float((er.err(got_sway, sway.hi, sway.lo) / sway.scale).max()), float((er.err(got_surge, surge.hi, surge.lo) / surge.scale).max()))
    _fixed(M_SWAY, RATIO_SWAY, worst, 2, "m_sway")


def test_replay_rows_extend_the_log():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_replay.npz"))
    for T in er.REPLAY_TS:
        X, t = er.replay_rows(g["Xs"], g["time"], T)
        assert X.shape == (T, 18) and t.shape == (T,) and (np.diff(t) > 0).all()
        n = min(T, 200)
        assert np.array_equal(X[:n], g["Xs"][:n]) and np.array_equal(t[:n], g["time"][:n])
