"""The marker fit on the GPU (rovmpc_fit_theta_gamma, rovmpc_fit_theta_gamma_device; law in include/rovmpc.h): the estimates
against the 50-digit minimiser of tests/fit_reference.py within the measured margin times each frame's conditioning scale, the
statuses, the bits' independence of the batch, the entry and the handle's dtype, the round trip through
rovmpc_transform_catenary, the state a controller is handed, and the refused arguments."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_reference as fr  # noqa: E402
from plan_controller_helpers import rv  # noqa: E402,F401
from plan_loop_helpers import same  # noqa: E402

pytestmark = pytest.mark.gpu

S = fr.Status


def engine(rv, up=1.0, dtype="f64", c_lo=fr.BRACKET[0]):
    return rv.Engine(rv.MPCConfig(N=1, K=1, dtype=dtype, c_lo=c_lo, c_hi=fr.BRACKET[1], L=fr.L_WS, frame="ENU" if up > 0 else "NED"))


def groups():
    """The scenes' indices by (up, M, max_iter): one call each."""
    g = {}
    for i, f in enumerate(fr.scenes()):
        g.setdefault((f.up, f.M, f.max_iter), []).append(i)
    return g


def inputs(idx):
    fs = [fr.scenes()[i] for i in idx]
    guess = np.array([(0.0, 0.0) if f.guess is None else f.guess for f in fs])
    return np.array([f.A for f in fs]), np.array([f.P for f in fs]), np.array([f.Y for f in fs]), guess


def rows_of(fit):
    return np.stack([np.asarray(c, dtype=np.float64) for c in fit], axis=1)


def rms0_error(k, rms0):
    """|rms0 - its 50-digit value| over the allowance of fit_reference.start_rms."""
    from mpmath import mp, mpf
    want, allow = fr.start_rms(k)
    with mp.workdps(fr.DPS):
        return float(abs(mpf(float(rms0)) - want)) / allow


def bulk():
    """The largest group: M = 16, ENU, the default max_iter."""
    return groups()[(1.0, 16, fr.MAX_ITER)]


@pytest.fixture(scope="module")
def gpu_rows(rv):
    """The fit of every scene, (B, 6), each group by one host-entry call."""
    out = np.empty((len(fr.scenes()), fr.OUT))
    for (up, M, max_iter), idx in groups().items():
        with engine(rv, up) as e:
            out[idx] = rows_of(e.fit_theta_gamma(*inputs(idx), max_iter=max_iter))
    return out


def test_converged_frames_against_the_reference(rv, gpu_rows):
    """theta^, gamma^ within M_FIT s of the 50-digit minimiser; rms within M_FIT s |J| plus one ulp."""
    n = 0
    for k, (f, r, g) in enumerate(zip(fr.scenes(), fr.references(), gpu_rows)):
        if r.status is not S.CONVERGED:
            continue
        assert S(int(g[5])) is S.CONVERGED, (f.name, g)
        ea = max(fr.angle_errors(g[0], g[1], r))
        er, ulp = fr.rms_error(g[2], r)
        print(f"{f.name:16s} trial steps {int(g[4]):2d} (NumPy {int(r.np_out[4]):2d}) error / scale: angle {ea / r.scale:.3g}, "
              f"rms {er / (r.scale * r.jnorm):.3g} (m = {fr.M_FIT})")
        assert ea <= fr.M_FIT * r.scale, (f.name, ea, r.scale)
        assert er <= fr.M_FIT * r.scale * r.jnorm + ulp, (f.name, er)
        assert rms0_error(k, g[3]) <= 1.0, f.name
        n += 1
    assert n >= 0.75 * len(gpu_rows)


def test_statuses_and_returned_starts(rv, gpu_rows):
    seen = set()
    for k, (f, r, g) in enumerate(zip(fr.scenes(), fr.references(), gpu_rows)):
        status = S(int(g[5]))
        assert status is r.status, (f.name, status, r.status)
        assert 0 <= g[4] <= f.max_iter and g[4] == int(g[4]), f.name
        seen.add(status)
        start = (0.0, 0.0) if f.guess is None else tuple(f.guess)
        if status is S.NONFINITE:
            assert np.isnan(g[:4]).all() and g[4] == 0, f.name
        elif status in (S.TOO_FEW, S.CHORD, S.DEGENERATE):
            assert (g[0], g[1]) == start and g[4] == 0 and same(g[2:3], g[3:4]), f.name
            assert rms0_error(k, g[3]) <= 1.0, f.name
        elif status is S.MAX_ITER:
            assert g[4] == f.max_iter == 1 and g[2] < g[3], f.name
    assert seen == set(S)


def test_max_iter_one_cuts_every_iterating_frame(rv, gpu_rows):
    idx = [i for i in bulk() if fr.references()[i].status is S.CONVERGED]
    with engine(rv) as e:
        fit = e.fit_theta_gamma(*inputs(idx), max_iter=1)
    assert np.all(fit.status == S.MAX_ITER) and np.all(fit.iters == 1)
    assert np.all(fit.rms < fit.rms0) and same(fit.rms0, gpu_rows[idx, 3])


def test_batch_independence(rv, gpu_rows):
    """Frame b of the B-frame call is bit-equal to the same frame alone, to the batch reversed and to the device entry."""
    idx = bulk()
    A, P, Y, G = inputs(idx)
    want = gpu_rows[idx]
    assert len(idx) > 8                                                      # more than one workgroup
    with engine(rv) as e:
        rev = rows_of(e.fit_theta_gamma(A[::-1], P[::-1], Y[::-1], G[::-1]))
        assert same(rev[::-1], want)
        dev = rows_of(e.fit_theta_gamma_device(A, P, Y, G))
        assert same(dev, want)
        for b in range(len(idx)):
            one = e.fit_theta_gamma(A[b], P[b], Y[b], G[b])
            assert np.ndim(one.theta) == 0
            assert same(np.array([float(c) for c in one]), want[b]), fr.scenes()[idx[b]].name
        # a null guess is the start (0, 0)
        zero = [b for b in range(len(idx)) if not G[b].any()]
        assert same(rows_of(e.fit_theta_gamma(A[zero], P[zero], Y[zero])), want[zero])
        # no frames: nothing to do
        empty = e.fit_theta_gamma(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 16, 3)))
        assert empty.theta.shape == (0,)


def test_fp32_handle_gives_the_same_bits(rv):
    """All arithmetic is double whatever the handle's dtype; L, c_lo, c_hi exact in float32 reach the kernel unchanged."""
    c_lo = float(np.float32(fr.BRACKET[0]))
    for v in (fr.L_WS, c_lo, fr.BRACKET[1]):
        assert float(np.float32(v)) == v
    idx = bulk()
    got = []
    for dtype in ("f64", "f32"):
        with engine(rv, dtype=dtype, c_lo=c_lo) as e:
            got.append(rows_of(e.fit_theta_gamma(*inputs(idx))))
    assert same(got[0], got[1])
    assert np.all(got[0][:, 5] == [fr.references()[i].status for i in idx])


def test_round_trip_through_transform_catenary(rv):
    """The points rovmpc_transform_catenary gives for (theta, gamma) at M = 16, fed back from (0, 0), recover the angles within
    M_FIT s.  The frames are the noise-free well-posed ones with (1 + kappa') / sigma <= 100: the transform's points are good
    to M_TETHER 2^-52 (1 + kappa') L each (tests/test_tether_gpu.py holds the same device functions to that), which moves the
    minimiser by at most sqrt(48) times that over sigma = 3.1e-14 (1 + kappa') / sigma <= 3.1e-12, inside M_FIT tol."""
    import tether_reference as tr
    pick = [i for i in bulk() if fr.scenes()[i].name in {f"g{k}" for k in fr.WELL_POSED}
            and (1.0 + fr.references()[i].mp.kappa) / fr.references()[i].sigma <= 100.0]
    assert len(pick) >= 8
    assert tr.M_TETHER * fr.EPS * fr.L_WS * 48 ** 0.5 * 100.0 <= fr.M_FIT * fr.TOL
    A, P, _, _ = inputs(pick)
    truth = np.array([fr.scenes()[i].truth for i in pick])
    with engine(rv) as e:
        out, npts, _ = e.transform_catenary(A, P, truth[:, 0], truth[:, 1], fr.L_WS, 16)
        assert np.all(npts == 16)
        fit = e.fit_theta_gamma(A, P, out[3])
    assert np.all(fit.status == S.CONVERGED)
    for k, i in enumerate(pick):
        bound = fr.M_FIT * fr.references()[i].scale
        assert abs(fit.theta[k] - truth[k, 0]) <= bound and abs(fit.gamma[k] - truth[k, 1]) <= bound, fr.scenes()[i].name
        kap = fr.references()[i].mp.kappa                                      # its points' rounding and the fit's own
        assert fit.rms[k] <= 2.0 * tr.M_TETHER * fr.EPS * (1.0 + kap) * fr.L_WS, fr.scenes()[i].name


def test_with_markers_feeds_a_controller(rv):
    """MPCState.with_markers replaces (theta, gamma) by the fit; an MPPI step from it is the step from the state built with
    theta^, gamma^ directly, bit for bit.  A fit that does not converge raises ValueError naming the status."""
    arr, _ = rv.synthetic_problem(64, 4)
    base = rv.MPCState(P0=arr[0:3], P1=arr[3:6], V1=arr[6:9], A1=arr[9:12], theta=0.0, gamma=0.0, theta_prev=arr[14], gamma_prev=arr[15])
    out, npts, _ = rv.default_engine().transform_catenary(arr[0:3], arr[3:6], arr[12], arr[13], 3.0, 16)
    assert np.all(npts == 16)
    markers = out[3, 0]
    fitted = base.with_markers(markers)
    fit = rv.fit_theta_gamma(base.P0, base.P1, markers)
    assert rv.FitStatus(int(fit.status)) is rv.FitStatus.CONVERGED and isinstance(fit, rv.CableFit)
    assert (fitted.theta, fitted.gamma) == (float(fit.theta), float(fit.gamma))
    assert abs(fitted.theta - arr[12]) < 1e-9 and abs(fitted.gamma - arr[13]) < 1e-9
    assert fitted.theta_prev == base.theta_prev and np.array_equal(fitted.P1, base.P1)
    direct = dataclasses.replace(base, theta=float(fit.theta), gamma=float(fit.gamma))
    us = []
    for state in (fitted, direct):
        ctl = rv.MPPI(N=4, K=64, seed=5)
        us.append(ctl.step(state))
        ctl.close()
    assert same(us[0], us[1])
    bad = markers.copy()
    bad[1:-1] = np.nan
    with pytest.raises(ValueError, match="TOO_FEW"):
        base.with_markers(bad)


def test_bad_arguments_are_refused(rv):
    f = fr.scenes()[0]
    A, P, Y = (np.ascontiguousarray(x) for x in (f.A[None], f.P[None], f.Y[None]))
    out = np.full((1, fr.OUT), 7.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    with engine(rv) as e:
        lib, h = e.lib, e._h
        dflt = rv.FitParams()
        lib.rovmpc_default_fit_params(C.byref(dflt))
        assert (dflt.struct_size, dflt.max_iter, dflt.tol) == (C.sizeof(rv.FitParams), fr.MAX_ITER, fr.TOL)

        def refused(word, P0=ptr(A), P1=ptr(P), Ym=ptr(Y), B=1, M=16, params=None, o=ptr(out)):
            for entry in (lib.rovmpc_fit_theta_gamma, lib.rovmpc_fit_theta_gamma_device):
                rc = entry(h, P0, P1, Ym, B, M, None, params, o)
                assert rc == -1 and word in lib.rovmpc_last_error(h).decode(), (word, lib.rovmpc_last_error(h))
            assert np.all(out == 7.0)

        def params(**kw):
            p = rv.FitParams.make()
            for k, v in kw.items():
                setattr(p, k, v)
            return C.byref(p)

        refused("null pointer", P0=None)
        refused("null pointer", P1=None)
        refused("null pointer", Ym=None)
        refused("null pointer", o=None)
        refused("M must", M=2)
        refused("M must", M=17)
        refused("B must", B=-1)
        refused("tol must", params=params(tol=-1e-9))
        refused("tol must", params=params(tol=np.nan))
        refused("max_iter", params=params(max_iter=0))
        refused("max_iter", params=params(max_iter=1001))
        refused("struct_size", params=params(struct_size=8))
        assert lib.rovmpc_fit_theta_gamma(None, ptr(A), ptr(P), ptr(Y), 1, 16, None, None, ptr(out)) == -1
        # B = 0 is fine and launches nothing, whatever the pointers
        assert lib.rovmpc_fit_theta_gamma(h, None, None, None, 0, 16, None, None, None) == 0
        assert lib.rovmpc_fit_theta_gamma_device(h, None, None, None, 0, 16, None, None, None) == 0
        with pytest.raises(ValueError):
            e.fit_theta_gamma(f.A, f.P, f.Y[:2])
        with pytest.raises(ValueError):
            e.fit_theta_gamma(f.A, f.P, f.Y, tol=-1.0)
        with pytest.raises(ValueError):
            e.fit_theta_gamma(f.A, f.P, f.Y, max_iter=0)
        # the defaults through a null params: the scene's own result
        assert lib.rovmpc_fit_theta_gamma(h, ptr(A), ptr(P), ptr(Y), 1, 16, None, None, ptr(out)) == 0
        assert same(out[0], rows_of(e.fit_theta_gamma(A, P, Y))[0])
