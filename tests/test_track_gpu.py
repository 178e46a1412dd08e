"""The marker tracker on the GPU (rovmpc_track_markers, rovmpc_track_markers_device; law in include/rovmpc.h) on the recordings
R1 .. R6 of tests/track_reference.py: the chain law bit for bit against rovmpc_fit_theta_gamma, the decisions against
track_np and the angles against the 50-digit minimiser, independence of the batch, the carry law over split calls and
launches, the device entry and the closed loop enqueued behind it, the fp32 handle, the refused arguments, CableTrack.rows."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_reference as fr  # noqa: E402
import track_reference as tk  # noqa: E402
from plan_controller_helpers import rv, defaults  # noqa: E402,F401
from plan_loop_helpers import same  # noqa: E402

pytestmark = pytest.mark.gpu

S, St = fr.Status, tk.State
NAN2 = (math.nan, math.nan)


def engine(rv, up=1.0, dtype="f64", **kw):
    return rv.Engine(rv.MPCConfig(N=1, K=1, dtype=dtype, c_lo=fr.BRACKET[0], c_hi=fr.BRACKET[1], L=fr.L_WS, frame="ENU" if up > 0 else "NED", **kw))


def rows_of(track):
    """A CableTrack as the entry's out (..., 9)."""
    return np.stack([np.asarray(c, dtype=np.float64) for c in (track.theta, track.gamma, track.theta_prev, track.gamma_prev, track.rms,
                                                             track.iters, track.status, track.state, track.start)], axis=-1)


def run(e, rec, carry="own", sl=slice(None), device=False, **kw):
    carry = rec.carry if isinstance(carry, str) else carry
    fn = e.track_markers_device if device else e.track_markers
    return fn(rec.A[sl], rec.P[sl], rec.Y[sl], carry=carry, starts=rec.starts, rms_max=rec.rms_max, **kw)


@pytest.fixture(scope="module")
def gpu_tracks(rv):
    """Every recording alone, by one host-entry call with its own parameters: (out (T, 9), carry (2,)) each."""
    got = []
    for rec in tk.recordings():
        with engine(rv, rec.up) as e:
            t = run(e, rec)
            got.append((rows_of(t), t.carry))
    return got


def check_chain(e, rec, out, carry_in):
    """Every attempt the law names, by rovmpc_fit_theta_gamma with that start as guess: theta, gamma, rms and status of the
    tracker's frame bit for bit, the step counts summed, the start taken from the tracker's own previous output."""
    T, n = len(rec.Y), len(rec.starts)
    c_in = np.array(NAN2 if carry_in is None else carry_in, dtype=np.float64)
    prev = np.concatenate([c_in[None], out[:-1, 0:2]])                      # the carry as frame t found it
    guess = np.concatenate([prev[:, None], np.broadcast_to(np.array(rec.starts), (T, n, 2))], axis=1)      # (T, 1 + n, 2)
    rep = lambda x: np.repeat(x, 1 + n, axis=0)
    fit = e.fit_theta_gamma(rep(rec.A), rep(rec.P), rep(rec.Y), guess.reshape(-1, 2))
    fit = np.stack([np.asarray(c, dtype=np.float64) for c in fit], axis=1).reshape(T, 1 + n, fr.OUT)
    for t in range(T):
        have = bool(np.isfinite(prev[t]).all())
        steps, accepted = 0, False
        for k in range(-1 if have else 0, n):
            r = fit[t, k + 1]
            steps += int(r[4])
            accepted = r[5] == S.CONVERGED and r[2] <= rec.rms_max
            if accepted or r[5] in (S.TOO_FEW, S.NONFINITE):
                break
        o = out[t]
        assert o[8] == k and o[6] == r[5] and o[5] == steps, (rec.name, t, o, r, steps)
        if accepted:
            assert same(o[[0, 1, 4]], r[[0, 1, 2]]), (rec.name, t, o, r)
            assert o[7] == (St.LOCKED if k < 0 else St.ACQUIRED)
        else:
            assert np.isnan(o[4]) and o[7] == (St.HELD if have else St.NONE)
            assert same(o[0:2], prev[t] if have else np.array(NAN2)), (rec.name, t)
        assert same(o[2:4], prev[t] if have else o[0:2]), (rec.name, t)


def test_chain_law(rv, gpu_tracks):
    for rec, (out, carry) in zip(tk.recordings(), gpu_tracks):
        with engine(rv, rec.up) as e:
            check_chain(e, rec, out, rec.carry)
        assert same(carry, out[-1, 0:2]), rec.name                           # the outgoing carry: the last frame's output


def test_against_the_reference(rv, gpu_tracks):
    """States, statuses, start indices and step counts are track_np's; accepted angles within M_FIT s of the minimiser."""
    for rec, (out, _), (ref, _), per in zip(tk.recordings(), gpu_tracks, tk.references(), tk.minimisers()):
        print(rec.name, "steps", out[:, 5].astype(int), "NumPy", ref[:, 5].astype(int))
        assert tuple(St(int(x)) for x in out[:, 7]) == rec.states, rec.name
        for col in (5, 6, 7, 8):
            assert np.array_equal(out[:, col], ref[:, col]), (rec.name, col, out[:, col], ref[:, col])
        for t, (m, scale) in per.items():
            ea = max(tk.angle_errors(out[t, 0], out[t, 1], m))
            print(f"  frame {t:2d} angle error / scale {ea / scale:.3g} (m = {fr.M_FIT})")
            assert ea <= fr.M_FIT * scale, (rec.name, t, ea, scale)


def padded(rec, T):
    """The recording with markerless frames appended up to T frames (they hold, or stay NONE)."""
    n = T - len(rec.Y)
    tile = lambda x: np.concatenate([x, np.repeat(x[-1:], n, axis=0)])
    Y = tile(rec.Y)
    Y[len(rec.Y):] = np.nan
    return tile(rec.A), tile(rec.P), Y


def test_batch_independence(rv, gpu_tracks):
    """One call cannot mix M, the frame or the parameters, so the five recordings with 16 markers in ENU (R1, R2, R4, R5, R6),
    padded to T = 14, run as one batch of B = 5 under the default parameters -- two workgroups, the second part-filled -- and
    R3 (M = 5, NED) as a batch of three with different carries.  Each recording alone gives the same bits, in either order,
    by either entry; the unpadded frames are the unpadded run's wherever the parameters agree."""
    recs = [r for r in tk.recordings() if r.M == 16 and r.up == 1.0]
    assert len(recs) == 5
    T = 14
    A, P, Y = (np.stack(x) for x in zip(*[padded(r, T) for r in recs]))
    carry = np.array([NAN2 if r.carry is None else r.carry for r in recs])
    with engine(rv) as e:
        batch = e.track_markers(A, P, Y, carry=carry)
        out = rows_of(batch)
        assert out.shape == (5, T, tk.OUT) and batch.carry.shape == (5, 2)
        rev = e.track_markers(A[::-1], P[::-1], Y[::-1], carry=carry[::-1])
        assert same(rows_of(rev)[::-1], out) and same(rev.carry[::-1], batch.carry)
        dev = e.track_markers_device(A, P, Y, carry=carry)
        assert same(rows_of(dev), out) and same(dev.carry, batch.carry)
        for b, rec in enumerate(recs):
            one = e.track_markers(A[b], P[b], Y[b], carry=carry[b])
            assert one.theta.shape == (T,) and one.carry.shape == (2,)
            assert same(rows_of(one), out[b]) and same(one.carry, batch.carry[b]), rec.name
            if math.isinf(rec.rms_max):
                want = gpu_tracks[[r.name for r in tk.recordings()].index(rec.name)][0]
                assert same(out[b, :len(want)], want), rec.name
    r3 = tk.recordings()[2]
    assert r3.M == 5 and r3.up == -1.0
    carries = np.array([NAN2, (0.05, -0.2), (0.6, 0.3)])
    with engine(rv, -1.0) as e:
        batch = e.track_markers(np.stack([r3.A] * 3), np.stack([r3.P] * 3), np.stack([r3.Y] * 3), carry=carries)
        for b in range(3):
            one = e.track_markers(r3.A, r3.P, r3.Y, carry=carries[b])
            assert same(rows_of(one), rows_of(batch)[b]) and same(one.carry, batch.carry[b])
        assert same(rows_of(batch)[0], gpu_tracks[2][0])


def test_carry_law(rv, gpu_tracks):
    """R1 as one call, as 5 + 9 frames, as 14 calls of one frame and in launches of 4 frames: the same out and final carry.
    A NaN carry is no carry."""
    r1 = tk.recordings()[0]
    want, c_want = gpu_tracks[0]
    T = len(r1.Y)
    with engine(rv) as e:
        for cuts in ([0, 5, T], list(range(T + 1))):
            c, parts = None, []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                t = run(e, r1, carry=c, sl=slice(lo, hi))
                parts.append(rows_of(t)); c = t.carry
            assert same(np.concatenate(parts), want) and same(c, c_want), cuts
        assert same(rows_of(run(e, r1, carry=NAN2)), want)
        assert same(rows_of(run(e, r1, carry=(math.nan, 0.25))), want)
        e.set_option("track_chunk", 4)
        for device in (False, True):
            t = run(e, r1, device=device)
            assert same(rows_of(t), want) and same(t.carry, c_want), device
            t = run(e, r1, carry=NAN2, device=device)                        # the carry buffer read by the first launch only
            assert same(rows_of(t), want) and same(t.carry, c_want), device
        for bad in (0, 65537, 2.5):
            with pytest.raises(rv.RovmpcError):
                e.set_option("track_chunk", bad)


def base_rows(recs, T):
    """State rows (B, T, 16) for the recordings' first T frames: P0, P1 theirs, a small velocity and acceleration, slots
    12..15 a sentinel."""
    rows = np.full((len(recs), T, 16), 7.0)
    for b, r in enumerate(recs):
        rows[b, :, 0:3], rows[b, :, 3:6] = r.A[:T], r.P[:T]
        rows[b, :, 6:9] = [0.05, -0.02, 0.01]
        rows[b, :, 9:12] = [0.0, 0.01, -0.01]
    return rows


def test_device_entry_fills_the_state_rows(rv, gpu_tracks):
    """d_exo: only slots 12..15 of the frames that are not NONE change, to out[..., 0:4]; R4 leaves it untouched."""
    for k in (0, 3, 5):                                                       # R1 (holds), R4 (NONE throughout), R6 (a gate)
        rec = tk.recordings()[k]
        rows = base_rows([rec], len(rec.Y))[0]
        rows[:, 12:16] = np.arange(4) + 100.0
        with engine(rv, rec.up) as e:
            track, got = run(e, rec, device=True, exo=rows)
        out = rows_of(track)
        assert same(out, gpu_tracks[k][0])
        want = rows.copy()
        ok = out[:, 7] != St.NONE
        want[ok, 12:16] = out[ok, 0:4]
        assert same(got, want), rec.name
        assert ok.any() != (rec.name == "R4")
        assert same(got, track.rows(rows, allow_missing=True))


def test_closed_loop_straight_behind_the_tracker(rv):
    """B = 2, T = 6: rovmpc_mppi_closed_loop_batch_device (feedback 0, K = 64, N = 4) on the d_exo the tracker fills, enqueued
    behind it with no synchronise between, gives the rows of the same loop on host-assembled rows, bit for bit."""
    import torch
    T, N = 6, 4
    recs = [tk.recordings()[1], tk.recordings()[0]]                          # R2 (an incoming carry) and R1 (none), 6 frames
    A, P, Y = (np.ascontiguousarray(np.stack([getattr(r, n)[:T] for r in recs])) for n in "APY")
    carry = np.array([recs[0].carry, NAN2])
    rows = base_rows(recs, T)
    dev = torch.device("cuda", 0)
    e = rv.Engine(rv.MPCConfig(N=N, K=64, c_lo=fr.BRACKET[0], c_hi=fr.BRACKET[1], L=fr.L_WS), rv.default_model())
    plan, std = defaults(rv, N)
    mp = rv.MPPIParams.make(1, 1.0, std)
    seeds = np.array([11, 12], dtype=np.uint64)
    track = e.track_markers(A, P, Y, carry=carry)
    assert np.all(track.state != St.NONE)
    host_rows = track.rows(rows)
    assert same(host_rows[..., :12], rows[..., :12]) and same(host_rows[..., 12], track.theta) and same(host_rows[..., 15], track.gamma_prev)
    W = e.mppi_row_len()

    def loop(d_exo, before=None):
        d_rows = torch.zeros((T, 2, W), dtype=torch.float64, device=dev)
        e.mppi_reset_batch(np.stack([plan, plan]))
        torch.cuda.synchronize(dev)
        if before:
            before()
        e.mppi_closed_loop_batch_device(d_exo.data_ptr(), T, False, seeds, 0, mp, d_rows.data_ptr())
        torch.cuda.synchronize(dev)
        return d_rows.cpu().numpy()

    want = loop(torch.tensor(host_rows, device=dev))
    d0, d1, dY, dC = (torch.tensor(x, device=dev) for x in (A, P, Y, carry))
    d_exo = torch.tensor(rows, device=dev)
    d_out = torch.empty((2, T, tk.OUT), dtype=torch.float64, device=dev)
    tp = rv.TrackParams.make()

    def tracker():
        assert e.lib.rovmpc_track_markers_device(e._h, d0.data_ptr(), d1.data_ptr(), dY.data_ptr(), 2, T, 16, dC.data_ptr(), C.byref(tp),
                                                 d_out.data_ptr(), d_exo.data_ptr()) == 0

    got = loop(d_exo, before=tracker)
    assert np.isfinite(want[..., 0]).all()
    assert same(got, want)
    assert same(d_exo.cpu().numpy(), host_rows) and same(d_out.cpu().numpy(), rows_of(track)) and same(dC.cpu().numpy(), track.carry)
    e.close()


def test_fp32_handle_obeys_the_chain_law(rv):
    r1 = tk.recordings()[0]
    with engine(rv, dtype="f32") as e:
        t = run(e, r1)
        check_chain(e, r1, rows_of(t), None)
        assert tuple(St(int(x)) for x in t.state) == r1.states


def test_bad_arguments_are_refused(rv):
    r5 = tk.recordings()[4]
    A, P, Y = (np.ascontiguousarray(x[None]) for x in (r5.A, r5.P, r5.Y))
    out = np.full((1, 1, tk.OUT), 7.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    with engine(rv) as e:
        lib, h = e.lib, e._h
        d = rv.TrackParams()
        lib.rovmpc_default_track_params(C.byref(d))
        assert (d.struct_size, d.n_starts, d.max_iter, d.tol, d.rms_max) == (C.sizeof(rv.TrackParams), 5, fr.MAX_ITER, fr.TOL, math.inf)
        assert tuple(tuple(s) for s in d.starts)[:5] == tk.STARTS
        host, device = lib.rovmpc_track_markers, lib.rovmpc_track_markers_device

        def refused(word, P0=ptr(A), P1=ptr(P), Ym=ptr(Y), B=1, T=1, M=16, params=None, o=ptr(out)):
            for rc in (host(h, P0, P1, Ym, B, T, M, None, params, o), device(h, P0, P1, Ym, B, T, M, None, params, o, None)):
                assert rc == -1 and word in lib.rovmpc_last_error(h).decode(), (word, lib.rovmpc_last_error(h))
            assert np.all(out == 7.0)

        def params(**kw):
            p = rv.TrackParams.make()
            for k, v in kw.items():
                if k == "start":
                    p.starts[v[0]][v[1]] = v[2]
                else:
                    setattr(p, k, v)
            return C.byref(p)

        for name in ("P0", "P1", "Ym", "o"):
            refused("null pointer", **{name: None})
        refused("B must", B=-1)
        refused("T must", T=-1)
        refused("M must", M=2)
        refused("M must", M=17)
        refused("struct_size", params=params(struct_size=16))
        refused("tol must", params=params(tol=-1e-9))
        refused("tol must", params=params(tol=math.nan))
        refused("max_iter", params=params(max_iter=0))
        refused("max_iter", params=params(max_iter=1001))
        refused("n_starts", params=params(n_starts=0))
        refused("n_starts", params=params(n_starts=9))
        refused("not finite", params=params(start=(2, 0, math.inf)))
        refused("not finite", params=params(start=(0, 1, math.nan)))
        refused("rms_max", params=params(rms_max=0.0))
        refused("rms_max", params=params(rms_max=-1.0))
        refused("rms_max", params=params(rms_max=math.nan))
        refused("2^24", B=4097, T=4096)
        refused("2^24", B=1, T=(1 << 24) + 1)
        assert host(None, ptr(A), ptr(P), ptr(Y), 1, 1, 16, None, None, ptr(out)) == -1
        assert device(None, ptr(A), ptr(P), ptr(Y), 1, 1, 16, None, None, ptr(out), None) == -1
        # a start beyond n_starts is not read
        assert host(h, ptr(A), ptr(P), ptr(Y), 1, 1, 16, None, params(start=(7, 0, math.nan)), ptr(out)) == 0
        out[:] = 7.0
        # no recordings or no frames: fine, nothing launched, whatever the pointers
        for B, T in ((0, 5), (5, 0), (0, 0)):
            assert host(h, None, None, None, B, T, 16, None, None, None) == 0
            assert device(h, None, None, None, B, T, 16, None, None, None, None) == 0
        assert np.all(out == 7.0)
        # the defaults through a null params: the recording's own result
        assert host(h, ptr(A), ptr(P), ptr(Y), 1, 1, 16, None, None, ptr(out)) == 0
        assert same(out[0], rows_of(run(e, r5)))
        for kw in (dict(starts=[]), dict(starts=[(0.0, 0.0)] * 9), dict(starts=[(0.0, math.inf)]), dict(rms_max=0.0), dict(tol=-1.0), dict(max_iter=0)):
            with pytest.raises(ValueError):
                e.track_markers(r5.A, r5.P, r5.Y, **kw)
        with pytest.raises(ValueError):
            e.track_markers(r5.A, r5.P, r5.Y[:, :2])
        empty = e.track_markers(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 16, 3)))
        assert empty.theta.shape == (0,) and np.isnan(empty.carry).all()


def test_cable_track_rows(rv, gpu_tracks):
    r1, r4 = tk.recordings()[0], tk.recordings()[3]
    with engine(rv) as e:
        t1 = e.track_markers(r1.A, r1.P, r1.Y)
    assert same(rows_of(t1), gpu_tracks[0][0])
    assert isinstance(t1, rv.CableTrack) and tuple(rv.TrackState(int(s)) for s in t1.state) == tuple(rv.TrackState(int(s)) for s in r1.states)
    rows = base_rows([r1], 14)[0]
    filled = t1.rows(rows)
    assert filled is not rows and np.all(rows[:, 12:16] == 7.0)
    assert same(filled[:, :12], rows[:, :12])
    for slot, col in zip(range(12, 16), (t1.theta, t1.gamma, t1.theta_prev, t1.gamma_prev)):
        assert same(filled[:, slot], col)
    with pytest.raises(ValueError):
        t1.rows(rows[:5])
    t4 = rv.track_markers(r4.A, r4.P, r4.Y)                                  # (the shared helper engine: L = 3 m, ENU, its own bracket)
    assert np.all(t4.state == rv.TrackState.NONE) and np.isnan(t4.carry).all()
    with pytest.raises(ValueError, match="NONE"):
        t4.rows(base_rows([r4], 3)[0])
    assert same(t4.rows(base_rows([r4], 3)[0], allow_missing=True), base_rows([r4], 3)[0])
    with engine(rv) as e:
        both = e.track_markers(np.stack([r4.A, r1.A[:3]]), np.stack([r4.P, r1.P[:3]]), np.stack([r4.Y, r1.Y[:3]]))
    got = both.rows(base_rows([r4, r1], 3), allow_missing=True)
    assert np.all(got[0, :, 12:16] == 7.0) and same(got[1, :, 12], t1.theta[:3])
