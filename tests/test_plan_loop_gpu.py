"""Device-resident closed loops of MPPI and CEM, single and batched (rovmpc_*_closed_loop_device / _closed_loop_batch_device)
against the host-stepped loop over the existing rovmpc_*_step / _step_batch entries, bit for bit: every row (record, plan,
spread, elite list, stats) of T = 12 control steps, the handle's state after the call, split calls, a poisoned problem in a
batch, no disturbance of the other entry points, determinism and the error codes.

The reference states are built by the plant rule (plan_loop_helpers.next_state, checked against closed_loop.state_of_step
in test_plan_loop_host.py) from the records the host loop itself returned; the measured rows are closed_loop_inputs(engine,
12, T).  No tolerance appears anywhere: ``same`` compares bit patterns, so rows that carry NaN compare too."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import defaults, rv  # noqa: E402,F401
from plan_loop_helpers import assert_rows_equal, host_loop, host_loop_batch, next_state, parts_of, record_of, same  # noqa: E402

pytestmark = pytest.mark.gpu

T = 12
_LAM = {}


def rows_for(rv, ctl, n=T, B=None):
    """closed_loop_inputs(engine, 12, n); for a batch B consecutive stretches of one longer trajectory: (B, n, 16)."""
    from rovmpc.closed_loop import closed_loop_inputs
    if B is None:
        return closed_loop_inputs(ctl.engine, 12, n)[0]
    return np.ascontiguousarray(closed_loop_inputs(ctl.engine, 12, B * n)[0].reshape(B, n, 16))


def plan_for(rv, N, b=0):
    mean, std = defaults(rv, N)
    return mean + 0.05 * std * np.random.default_rng(1000 + 7 * b + N).standard_normal((N, 3)), std


def seed_of(b):
    return 1000003 * (b + 1) + 17


def lam_for(rv, cfg_kw, model):
    """A temperature on the scale of the spread of one draw's costs, so that the weights neither collapse nor flatten."""
    key = tuple(sorted(cfg_kw.items()))              # (every test here runs the default model)
    if key not in _LAM:
        nominal, std = plan_for(rv, cfg_kw["N"])
        m = rv.MPPI(rv.MPCConfig(**cfg_kw), model, lam=1.0, std=std, n_iter=1, nominal=nominal)
        m.step(rows_for(rv, m, 1)[0])
        J = np.asarray(m.engine.mppi_last()[1], dtype=np.float64)
        m.close()
        J = J[np.isfinite(J)]
        _LAM[key] = float(max(np.median(J - J.min()), 1e-12)) if len(J) else 1.0
    return _LAM[key]


def make_mppi(rv, cfg_kw, n_iter, model=None, b=0):
    model = model or rv.default_model()
    nominal, std = plan_for(rv, cfg_kw["N"], b)
    return rv.MPPI(rv.MPCConfig(**cfg_kw), model, lam=lam_for(rv, cfg_kw, model), std=std, n_iter=n_iter, seed=seed_of(b), nominal=nominal)


def cem_kw(rv, N, n_iter, n_elite):
    mean0, std = defaults(rv, N)
    return dict(n_elite=n_elite, n_iter=n_iter, alpha=0.15, std=std, std_min=0.02 * std, lo=mean0[0] - 1.2 * std, hi=mean0[0] + 0.9 * std)


def make_cem(rv, cfg_kw, n_iter, n_elite, model=None, b=0):
    return rv.CEM(rv.MPCConfig(**cfg_kw), model or rv.default_model(), seed=seed_of(b), mean=plan_for(rv, cfg_kw["N"], b)[0],
                  **cem_kw(rv, cfg_kw["N"], n_iter, n_elite))


def last_of(ctl, cem):
    return ctl.engine.cem_last() if cem else ctl.engine.mppi_last()


def check_single(rv, make, cem, feedback, n=T, finite=False):
    """One device loop against the host-stepped loop, then the state both left behind: last candidates and costs, the
    Python plan, and the next step."""
    dev, ref = make(), make()
    rows = rows_for(rv, dev, n + 1)
    res = dev.run(rows[:n], feedback)
    want, states = host_loop(ref, rows[:n], feedback, cem)
    what = ("cem" if cem else "mppi", feedback)
    if finite:
        print("J* of the loop:", res.records[:, 0])
        assert np.isfinite(res.records[:, 0]).all(), what
    assert_rows_equal(res, want, what)
    assert dev.step_count == ref.step_count == n
    (Ud, Jd), (Uh, Jh) = last_of(dev, cem), last_of(ref, cem)
    assert same(Ud, Uh) and same(Jd, Jh), what
    for name in (("mean", "std", "elites") if cem else ("nominal",)):
        assert same(getattr(dev, name), getattr(ref, name)), (what, name)
    assert same(record_of(dev.last), record_of(ref.last)), what
    st = next_state(rows[n], states[-1], want["records"][-1], feedback)
    ud, uh = dev.step(st), ref.step(st)
    assert same(ud, uh) and same(record_of(dev.last), record_of(ref.last)), what
    for name in (("mean", "std", "elites") if cem else ("nominal",)):
        assert same(getattr(dev, name), getattr(ref, name)), (what, name, "after the next step")
    dev.close(); ref.close()
    return res


# ---- MPPI: four update workgroups (K = 256), so the finishing workgroup is decided by the ticket -------------------------
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("n_iter", [1, 2])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mppi_loop(rv, dtype, n_iter, feedback):
    cfg_kw = dict(N=6, K=256, dtype=dtype)
    check_single(rv, lambda: make_mppi(rv, cfg_kw, n_iter), False, feedback, finite=not feedback)


# ---- CEM: one workgroup (K = 256, E = 16), finite box ----------------------------------------------------------------------
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("n_iter", [1, 2])
def test_cem_loop(rv, n_iter, feedback):
    cfg_kw = dict(N=6, K=256)
    res = check_single(rv, lambda: make_cem(rv, cfg_kw, n_iter, 16), True, feedback, finite=not feedback)
    lo, hi = cem_kw(rv, 6, n_iter, 16)["lo"], cem_kw(rv, 6, n_iter, 16)["hi"]
    assert (res.u >= lo).all() and (res.u <= hi).all()
    assert res.elites.dtype == np.int64 and res.elites.shape == (T, 16) and (res.elites[res.elites >= 0] < 256).all()


def test_cem_loop_f32(rv):
    check_single(rv, lambda: make_cem(rv, dict(N=6, K=256, dtype="f32"), 2, 16), True, True)


def test_cem_loop_two_workgroups(rv):
    """K = 8192, E = 64: the cross-workgroup select, the hand-off on the workgroup that finishes it."""
    check_single(rv, lambda: make_cem(rv, dict(N=6, K=8192), 2, 64), True, True)


# ---- rows wider than the update's workgroup (3 N > 256: the other template instance) --------------------------------------
def test_mppi_loop_wide_rows(rv):
    check_single(rv, lambda: make_mppi(rv, dict(N=100, K=64), 2), False, True)


def test_cem_loop_wide_rows(rv):
    check_single(rv, lambda: make_cem(rv, dict(N=100, K=64), 2, 8), True, True)


# ---- model paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["no_builtin", "force_interpreter"])
@pytest.mark.parametrize("cem", [False, True])
def test_model_paths(rv, cem, path):
    cfg_kw = dict(N=6, K=256, **{path: True})
    make = (lambda: make_cem(rv, cfg_kw, 2, 16)) if cem else (lambda: make_mppi(rv, cfg_kw, 2))
    probe = make()
    assert probe.engine.model_path == {"no_builtin": "jit", "force_interpreter": "interpreter"}[path]
    probe.close()
    check_single(rv, make, cem, True, n=6)


# ---- batched ----------------------------------------------------------------------------------------------------------------
def make_batch(rv, cfg_kw, cem, B, n_iter=2, n_elite=16, same_problem=False):
    model = rv.default_model()
    plans = np.stack([plan_for(rv, cfg_kw["N"], 0 if same_problem else b)[0] for b in range(B)])
    seeds = [seed_of(0 if same_problem else b) for b in range(B)]
    if cem:
        return rv.BatchedCEM(rv.MPCConfig(**cfg_kw), model, B=B, seeds=seeds, mean=plans, **cem_kw(rv, cfg_kw["N"], n_iter, n_elite))
    return rv.BatchedMPPI(rv.MPCConfig(**cfg_kw), model, B=B, lam=lam_for(rv, cfg_kw, model), std=plan_for(rv, cfg_kw["N"])[1],
                          n_iter=n_iter, seeds=seeds, nominal=plans)


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("cem", [False, True])
def test_batched_loop(rv, cem, B, feedback):
    """Every problem's T rows equal its own single-problem device loop and the host-stepped batched loop; then the state
    the two batched handles are left in."""
    cfg_kw = dict(N=6, K=256)
    dev, ref = make_batch(rv, cfg_kw, cem, B), make_batch(rv, cfg_kw, cem, B)
    rows = rows_for(rv, dev, T, B)
    res = dev.run(rows, feedback)
    assert res.records.shape[:2] == (T, B)
    assert_rows_equal(res, host_loop_batch(ref, rows, feedback, cem), ("batch", cem, B, feedback))
    for b in range(B):
        one = make_cem(rv, cfg_kw, 2, 16, b=b) if cem else make_mppi(rv, cfg_kw, 2, b=b)
        assert_rows_equal(one.run(rows[b], feedback), parts_of(res, np.s_[:, b]), ("single", cem, b, feedback))
        one.close()
    (Ud, Jd), (Uh, Jh) = dev.candidates(), ref.candidates()
    assert same(Ud, Uh) and same(Jd, Jh)
    for name in (("mean", "std", "elites") if cem else ("nominal",)):
        assert same(getattr(dev, name), getattr(ref, name)), name
    assert dev.step_count == ref.step_count == T
    st = rows[:, -1] * 1.0
    assert same(dev.step(st), ref.step(st)) and same(dev.records, ref.records)
    dev.close(); ref.close()


@pytest.mark.parametrize("cem", [False, True])
def test_batched_broadcast(rv, cem):
    """(T, 16) given to every problem equals B copies of it."""
    cfg_kw = dict(N=6, K=256)
    a, b = make_batch(rv, cfg_kw, cem, 3), make_batch(rv, cfg_kw, cem, 3)
    rows = rows_for(rv, a)
    ra, rb = a.run(rows, True), b.run(np.stack([rows] * 3), True)
    assert_rows_equal(ra, rb, "broadcast")
    a.close(); b.close()


@pytest.mark.parametrize("cem", [False, True])
def test_poisoned_problem(rv, cem):
    """Problem 1's measured rows are NaN from step 4 on: no finite cost from there, its plan stays put (shifted as every kept
    plan is), and the other two problems' rows are what they are without the poison."""
    cfg_kw, B, bad, t0 = dict(N=6, K=256), 3, 1, 4
    clean, pois = make_batch(rv, cfg_kw, cem, B), make_batch(rv, cfg_kw, cem, B)
    rows = rows_for(rv, clean, T, B)
    prow = rows.copy()
    prow[bad, t0:] = np.nan
    rc, rp = clean.run(rows, False), pois.run(prow, False)
    for b in (0, 2):
        assert_rows_equal(parts_of(rp, np.s_[:, b]), parts_of(rc, np.s_[:, b]), ("untouched", b))
    assert_rows_equal(parts_of(rp, np.s_[:t0, bad]), parts_of(rc, np.s_[:t0, bad]), "before the poison")
    assert not np.isfinite(rp.records[t0:, bad, 0]).any()
    assert np.isfinite(rp.records[:t0, bad, 0]).all()
    N = cfg_kw["N"]
    shift = np.minimum(np.arange(N) + 1, N - 1)
    for t in range(t0, T):
        assert same(rp.plans[t, bad], rp.plans[t - 1, bad][shift]), t       # plan* = the kept plan, bit for bit
    if cem:
        assert (rp.elites[t0:, bad] == -1).all() and (rp.stats[t0:, bad, 2] == 0).all() and np.isnan(rp.stats[t0:, bad, 0]).all()
    else:
        assert np.isnan(rp.stats[t0:, bad, 0]).all() and (rp.stats[t0:, bad, 1:3] == 0).all()
    clean.close(); pois.close()


# ---- split calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cem", [False, True])
def test_split_without_feedback_equals_one_call(rv, cem):
    cfg_kw = dict(N=6, K=256)
    make = (lambda: make_cem(rv, cfg_kw, 2, 16)) if cem else (lambda: make_mppi(rv, cfg_kw, 2))
    one, two = make(), make()
    rows = rows_for(rv, one)
    whole, first, second = one.run(rows, False), two.run(rows[:5], False), two.run(rows[5:], False)
    assert two.step_count == T
    a, b = parts_of(first), parts_of(second)
    assert_rows_equal(whole, {k: np.concatenate([a[k], b[k]]) for k in a}, "5 + 7")
    one.close(); two.close()


@pytest.mark.parametrize("cem", [False, True])
def test_split_with_feedback_restarts_from_its_first_row(rv, cem):
    """With feedback each call starts from its own exo[0]: 5 + 7 equals a host loop whose fed-back angles restart at row 5."""
    cfg_kw = dict(N=6, K=256)
    make = (lambda: make_cem(rv, cfg_kw, 2, 16)) if cem else (lambda: make_mppi(rv, cfg_kw, 2))
    dev, ref = make(), make()
    rows = rows_for(rv, dev)
    for part in (rows[:5], rows[5:]):
        assert_rows_equal(dev.run(part, True), host_loop(ref, part, True, cem)[0], ("split", len(part)))
    dev.close(); ref.close()


# ---- determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cem", [False, True])
def test_same_call_twice(rv, cem):
    cfg_kw = dict(N=6, K=256)
    ctl = make_cem(rv, cfg_kw, 2, 16) if cem else make_mppi(rv, cfg_kw, 2)
    rows, plan = rows_for(rv, ctl), plan_for(rv, 6)[0]
    a = ctl.run(rows, True)
    ctl.reset(plan); ctl.step_count = 0
    b = ctl.run(rows, True)
    assert_rows_equal(a, b, "twice")
    ctl.close()


# ---- the other entry points, before and after a plan loop on the same handle -----------------------------------------------
def test_other_entry_points_undisturbed(rv):
    import torch
    from rovmpc.closed_loop import closed_loop_pools, run_closed_loop
    cfg_kw = dict(N=6, K=256)
    ctl = make_mppi(rv, cfg_kw, 2)
    eng = ctl.engine
    dev = torch.device("cuda", 0)
    state, U = rv.synthetic_problem(256, 6)
    mean, std = defaults(rv, 6)
    pools = closed_loop_pools(eng, 2)
    Ub = torch.tensor(np.stack([U, U[::-1].copy()]), device=dev)
    stb = torch.tensor(np.stack([state, state * 1.01]), device=dev)

    def others():
        r = eng.step(state, U)
        rec = eng.mpc_step_sampled(state, 5, 3, mean[0], std, False).copy()
        out = torch.empty((2, eng.result_len), dtype=torch.float64, device=dev)
        eng.step_batch_device(2, stb.data_ptr(), Ub.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rep = run_closed_loop(eng, 12, 4, pools=pools, feedback=True)
        return [record_of(r), rec, out.cpu().numpy(), rep.u, rep.theta_gamma, rep.cost]

    before = others()
    rows = rows_for(rv, ctl)
    ctl.run(rows, True)
    eng.cem_reset(plan_for(rv, 6)[0])
    p = rv.CEMParams.make(**{k: (tuple(v) if isinstance(v, np.ndarray) else v) for k, v in cem_kw(rv, 6, 2, 16).items()})
    d_exo = torch.tensor(rows, device=dev)
    d_rows = torch.empty((T, eng.cem_row_len(16)), dtype=torch.float64, device=dev)
    eng.cem_closed_loop_device(d_exo.data_ptr(), T, True, 9, 0, p, d_rows.data_ptr())
    after = others()
    for a, b in zip(before, after):
        assert same(a, b)
    ctl.close()


# ---- errors: each returns its code before anything is launched, and the handle still works ----------------------------------
def test_errors(rv):
    import torch
    INVALID, UNSUPPORTED = -1, -4
    cfg_kw = dict(N=6, K=256)
    eng = rv.Engine(rv.MPCConfig(**cfg_kw), rv.default_model())
    lib, h = eng.lib, eng._h
    dev = torch.device("cuda", 0)
    rows = rows_for(rv, type("E", (), {"engine": eng})())
    d_exo = torch.tensor(np.stack([rows, rows]), device=dev)
    d_rows = torch.zeros((T, 2, eng.cem_row_len(16)), dtype=torch.float64, device=dev)
    ex, out = d_exo.data_ptr(), d_rows.data_ptr()
    _, std = defaults(rv, 6)
    mp = rv.MPPIParams.make(2, 1.0, std)
    cp = rv.CEMParams.make(**{k: (tuple(v) if isinstance(v, np.ndarray) else v) for k, v in cem_kw(rv, 6, 2, 16).items()})
    seeds = np.array([3, 4], dtype=np.uint64)
    sp = seeds.ctypes.data_as(C.c_void_p)
    single = ((lib.rovmpc_mppi_closed_loop_device, mp), (lib.rovmpc_cem_closed_loop_device, cp))
    batch = ((lib.rovmpc_mppi_closed_loop_batch_device, mp), (lib.rovmpc_cem_closed_loop_batch_device, cp))
    # before the matching reset
    for fn, p in single:
        assert fn(h, ex, T, 0, 1, 0, C.byref(p), out) == INVALID
    for fn, p in batch:
        assert fn(h, 2, ex, T, 0, sp, 0, C.byref(p), out) == INVALID
    plan = plan_for(rv, 6)[0]
    eng.mppi_reset(plan); eng.cem_reset(plan)
    eng.mppi_reset_batch(np.stack([plan, plan])); eng.cem_reset_batch(np.stack([plan, plan]))
    bad_m, bad_c = rv.MPPIParams.make(2, 1.0, std), rv.CEMParams.make(**{k: (tuple(v) if isinstance(v, np.ndarray) else v) for k, v in cem_kw(rv, 6, 2, 16).items()})
    bad_m.struct_size -= 8; bad_c.struct_size -= 8
    range_m, range_c = rv.MPPIParams.make(2, 1.0, std), rv.CEMParams.make(**{k: (tuple(v) if isinstance(v, np.ndarray) else v) for k, v in cem_kw(rv, 6, 2, 16).items()})
    range_m.lambda_ = -1.0; range_c.n_elite = 257
    for (fn, p), bad, rng in zip(single, (bad_m, bad_c), (range_m, range_c)):
        assert fn(None, ex, T, 0, 1, 0, C.byref(p), out) == INVALID
        assert fn(h, None, T, 0, 1, 0, C.byref(p), out) == INVALID
        assert fn(h, ex, T, 0, 1, 0, C.byref(p), None) == INVALID
        assert fn(h, ex, T, 0, 1, 0, None, out) == INVALID
        assert fn(h, ex, 0, 0, 1, 0, C.byref(p), out) == INVALID
        assert fn(h, ex, -3, 0, 1, 0, C.byref(p), out) == INVALID
        assert fn(h, ex, T, 2, 1, 0, C.byref(p), out) == INVALID
        assert fn(h, ex, T, -1, 1, 0, C.byref(p), out) == INVALID
        assert fn(h, ex, T, 0, 1, 0, C.byref(bad), out) == INVALID
        assert fn(h, ex, T, 0, 1, 0, C.byref(rng), out) == INVALID
        assert lib.rovmpc_last_error(h)
    for (fn, p), bad, rng in zip(batch, (bad_m, bad_c), (range_m, range_c)):
        assert fn(None, 2, ex, T, 0, sp, 0, C.byref(p), out) == INVALID
        assert fn(h, 2, None, T, 0, sp, 0, C.byref(p), out) == INVALID
        assert fn(h, 2, ex, T, 0, None, 0, C.byref(p), out) == INVALID
        assert fn(h, 2, ex, T, 0, sp, 0, C.byref(p), None) == INVALID
        assert fn(h, 2, ex, T, 0, sp, 0, None, out) == INVALID
        assert fn(h, 2, ex, 0, 0, sp, 0, C.byref(p), out) == INVALID
        assert fn(h, 2, ex, T, 2, sp, 0, C.byref(p), out) == INVALID
        assert fn(h, 3, ex, T, 0, sp, 0, C.byref(p), out) == INVALID          # a B other than the reset's
        assert fn(h, 0, ex, T, 0, sp, 0, C.byref(p), out) == INVALID
        assert fn(h, 2, ex, T, 0, sp, 0, C.byref(bad), out) == INVALID
        assert fn(h, 2, ex, T, 0, sp, 0, C.byref(rng), out) == INVALID
    assert not d_rows.cpu().numpy().any()                                    # nothing was launched
    assert lib.rovmpc_mppi_row_len(None) == 0 and lib.rovmpc_cem_row_len(h, 0) == 0 and lib.rovmpc_cem_row_len(h, 1025) == 0
    R = eng.result_len
    assert eng.mppi_row_len() == R + 18 + 4 and eng.cem_row_len(16) == R + 36 + 4 + 16
    # the handle still works: one good step of each, one good loop
    rec, _, _ = eng.mppi_step(rows[0], 1, 0, mp)
    assert np.isfinite(rec[0])
    rec = eng.cem_step(rows[0], 1, 0, cp)[0]
    assert np.isfinite(rec[0])
    for fn, p in single:
        assert fn(h, ex, T, 1, 1, 1, C.byref(p), out) == 0
    for fn, p in batch:
        assert fn(h, 2, ex, T, 1, sp, 0, C.byref(p), out) == 0
    eng.close()


def test_unsupported_with_a_communicator(rv):
    """Once rovmpc_comm_init has run the loops answer ROVMPC_ERR_UNSUPPORTED (world = 1: no peer is needed)."""
    import torch
    eng = rv.Engine(rv.MPCConfig(N=6, K=256), rv.default_model())
    plan, std = plan_for(rv, 6)
    eng.mppi_reset(plan); eng.cem_reset(plan)
    eng.mppi_reset_batch(plan[None]); eng.cem_reset_batch(plan[None])
    eng.comm_init(eng.comm_unique_id(), 0, 1)
    rows = rows_for(rv, type("E", (), {"engine": eng})())
    d_exo = torch.tensor(rows, device="cuda:0")
    d_rows = torch.zeros((T, eng.cem_row_len(16)), dtype=torch.float64, device="cuda:0")
    mp = rv.MPPIParams.make(1, 1.0, std)
    cp = rv.CEMParams.make(**{k: (tuple(v) if isinstance(v, np.ndarray) else v) for k, v in cem_kw(rv, 6, 1, 16).items()})
    seeds = np.array([3], dtype=np.uint64)
    sp = seeds.ctypes.data_as(C.c_void_p)
    lib, h = eng.lib, eng._h
    assert lib.rovmpc_mppi_closed_loop_device(h, d_exo.data_ptr(), T, 0, 1, 0, C.byref(mp), d_rows.data_ptr()) == -4
    assert lib.rovmpc_cem_closed_loop_device(h, d_exo.data_ptr(), T, 0, 1, 0, C.byref(cp), d_rows.data_ptr()) == -4
    assert lib.rovmpc_mppi_closed_loop_batch_device(h, 1, d_exo.data_ptr(), T, 0, sp, 0, C.byref(mp), d_rows.data_ptr()) == -4
    assert lib.rovmpc_cem_closed_loop_batch_device(h, 1, d_exo.data_ptr(), T, 0, sp, 0, C.byref(cp), d_rows.data_ptr()) == -4
    assert not d_rows.cpu().numpy().any()
    eng.comm_destroy()
    eng.close()


def test_run_plan_closed_loop(rv):
    """The driver: closed_loop_inputs rows, one call, a ClosedLoopReport equal to the host-stepped loop's figures."""
    from rovmpc.closed_loop import run_plan_closed_loop
    cfg_kw = dict(N=6, K=256)
    dev, ref = make_mppi(rv, cfg_kw, 1), make_mppi(rv, cfg_kw, 1)
    rep = run_plan_closed_loop(dev, 12, T, feedback=True)
    want, _ = host_loop(ref, rows_for(rv, ref), True)
    assert rep.steps == T and same(rep.u, want["records"][:, 2:5]) and same(rep.cost, want["records"][:, 0])
    assert same(rep.theta_gamma[1:], want["records"][:, 7:9]) and same(rep.theta_gamma[0], want["records"][0, 5:7])
    assert np.array_equal(rep.index, want["records"][:, 1].astype(np.int64))
    dev.close(); ref.close()
