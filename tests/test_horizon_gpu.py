"""rovmpc_score_pairs / rovmpc_score_pairs_device on the GPU (law in include/rovmpc.h) on the fixtures of tests/horizon_reference.py:
the metric law from the GPU's own pred bits, pred against 50 digits, the ties to rovmpc_replay and to the rollout, independence
of the batch, the edge shapes, the refusals, select_model(horizon=...)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import horizon_reference as hr  # noqa: E402
from horizon_reference import same  # noqa: E402
from plan_controller_helpers import rv, orc, oracle_cfg, oracle_model  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SLOT_FREE = ("x3*x5 - 0.5*x2", "sin(x1) + x7*x0")           # rows that read no named slot


def run(rv, fx, **kw):
    args = dict(fx.kwargs(), return_pred=True)
    args.update(kw)
    return rv.score_pairs(fx.theta_rows, fx.gamma_rows, fx.X, fx.time, fx.theta, fx.gamma, fx.mean, fx.scale, **args)


@pytest.fixture(scope="module")
def gpu(rv):
    """PairSkill of a fixture, computed once."""
    cache = {}

    def get(fx):
        if fx.name not in cache:
            cache[fx.name] = run(rv, fx)
        return cache[fx.name]
    return get


def all_fixtures():
    return [hr.fixture_a()] + hr.b_fixtures()


# ---- 1. the metric law ----------------------------------------------------------------------------------------------------------
def test_columns_follow_the_law_from_the_gpus_own_pred_bits(gpu):
    for fx in all_fixtures():
        sk = gpu(fx)
        table = sk.table()
        W = hr.n_windows(fx.X.shape[1], fx.H, fx.stride)
        assert sk.pred.shape == (len(fx.pairs), len(fx.lengths), W, fx.H, 2)
        for q in range(len(fx.pairs)):
            for b, n in enumerate(fx.lengths):
                ref = hr.skill_from_pred(sk.pred[q, b], fx.theta[b], fx.gamma[b], n, fx.H, fx.stride)
                assert same(table[q, b][:, 2:], ref[:, 2:]), (fx.name, q, b)
                bound = hr.column_bounds(ref, n)
                assert same(np.isnan(table[q, b]), np.isnan(ref)), (fx.name, q, b)
                assert (np.nan_to_num(np.abs(table[q, b] - ref)) <= bound).all(), (fx.name, q, b)


# ---- 2. the values against 50 digits ----------------------------------------------------------------------------------------------
def test_pred_is_within_four_times_the_references_own_error(gpu):
    b = hr.bounds()
    worst, where = hr.measure(lambda fx, q, k: gpu(fx).pred[q, k])
    print("GPU: largest |error| / (u S) = %.4g at %s (horizon_np: %g; allowed %g)" % (worst, where, b["np_figure"], hr.GPU_MARGIN * b["np_figure"]))
    assert worst <= hr.GPU_MARGIN * b["np_figure"], where


def test_pred_agrees_with_numpy_everywhere(gpu):
    """Every pair and window, not only the windows of the 50-digit runs: against horizon_np at 1e-9 of the entry's size where
    both are finite; the same entries are finite."""
    for fx in all_fixtures():
        sk = gpu(fx)
        for q in range(0, len(fx.pairs), 7 if fx.name == "A" else 1):
            for b, n in enumerate(fx.lengths):
                ref = fx.np_pair(q, b)[1]
                got = sk.pred[q, b, :len(ref)]
                fin = np.isfinite(ref)
                assert (np.isfinite(got) == fin).all(), (fx.name, q, b)
                big = np.abs(ref) > 1e6                                   # (a pair that blows up: the chain amplifies the last bits)
                np.testing.assert_allclose(got[fin & ~big], ref[fin & ~big], rtol=1e-9, atol=1e-9, err_msg=str((fx.name, q, b)))


# ---- 3. the replay tie --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ["rk4", "euler"])
def test_a_single_window_of_slot_free_rows_is_the_replay_bit_for_bit(rv, integ):
    fa = hr.fixture_a()
    fb = hr.fixture_b(5, 1)
    m = rv.DynamicsModel(np.zeros(18), np.ones(18), *SLOT_FREE)
    with rv.Engine(rv.MPCConfig(N=1, K=1, force_interpreter=True), m) as e:
        for X, time, n in ((fa.X[0], fa.time[0], 200), (fb.X[5], fb.time[5], 2 * hr.TILE + 8), (fb.X[5], fb.time[5], 3)):
            T = X.shape[0]
            th0, ga0 = 0.3, -0.2
            want_t, want_g = e.replay(X[:n], time[:n], th0, ga0, rv.RK4 if integ == "rk4" else rv.EULER)
            sk = rv.score_pairs([SLOT_FREE[0]], [SLOT_FREE[1]], X, time, np.full(T, th0), np.full(T, ga0), fa.mean, fa.scale, horizon=n - 1,
                                integrator=integ, lengths=[n], return_pred=True)
            assert sk.windows[0] == 1
            assert same(sk.pred[0, 0, 0, :, 0], want_t[1:]) and same(sk.pred[0, 0, 0, :, 1], want_g[1:]), (integ, n)


# ---- 4. the rollout tie -------------------------------------------------------------------------------------------------------------
def test_window_zero_is_the_rollout_of_the_same_controls(rv, orc):
    """A recording whose exogenous rows are those of the oracle's rollout_scalar (VT_NONE, uniform dt, default model, N = 8, one
    control sequence): the window from the state's node, the library's own rollout trajectory and the oracle agree at 1e-9."""
    N = 8
    cfg = rv.MPCConfig(N=N, K=1, vt_mode=rv.VT_NONE)
    state, U = rv.synthetic_problem(1, N)
    state = np.array(state, dtype=np.float64)
    state[14], state[15] = state[12] - 0.01, state[13] + 0.02            # a previous node that is not the node
    model = rv.default_model()
    ocfg, omodel = oracle_cfg(orc, cfg), oracle_model(orc, model)
    _, trajo, _ = orc.rollout_scalar(ocfg, omodel, orc.MPCState.from_array(state), U)
    with rv.Engine(cfg, model) as e:
        res = e.step(state, U)
    np.testing.assert_allclose(res.traj, trajo[0], rtol=1e-9, atol=1e-13)
    # rows 1 .. N + 1 of the recording are nodes 0 .. N of the rollout; row 0 is the previous node
    mean, scale = np.asarray(model.mean, float), np.asarray(model.scale, float)
    h = cfg.dt
    P0, P, V, A = state[0:3], state[3:6].copy(), state[6:9].copy(), state[9:12].copy()
    rows = [orc._exo_features_scalar(P0, P, V, A, mean, scale, 0)]
    for n in range(N):
        Vn = U[0, n].copy()
        P, A, V = P + (cfg.v_scale * h) * U[0, n], (Vn - V) / h, Vn
        rows.append(orc._exo_features_scalar(P0, P, V, A, mean, scale, 0))
    X = np.full((N + 2, 18), np.nan)                                     # the named slots are never read: NaN there is harmless
    X[1:, :14] = np.array(rows)
    X[0, :14] = X[1, :14]
    time = h * np.arange(N + 2)
    theta, gamma = np.full(N + 2, state[12]), np.full(N + 2, state[13])
    theta[0], gamma[0] = state[14], state[15]
    sk = rv.score_pairs([model.expr_theta], [model.expr_gamma], X, time, theta, gamma, mean, scale, horizon=N, return_pred=True)
    assert sk.windows[0] == 2
    np.testing.assert_allclose(sk.pred[0, 0, 1], trajo[0, 1:], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(sk.pred[0, 0, 1], res.traj[1:], rtol=1e-9, atol=1e-13)


# ---- 5. independence to the bit -----------------------------------------------------------------------------------------------------
def test_a_pair_alone_equals_the_pair_among_all_and_orders_do_not_matter(rv, gpu):
    fx = hr.fixture_a()
    whole = gpu(fx)
    for q in (0, fx.chosen, len(fx.pairs) - 1):
        it, ig = fx.pairs[q]
        alone = rv.score_pairs([fx.theta_rows[it]], [fx.gamma_rows[ig]], fx.X[0], fx.time[0], fx.theta[0], fx.gamma[0], fx.mean, fx.scale,
                               fx.H, return_pred=True)
        assert same(alone.table()[0], whole.table()[q]) and same(alone.pred[0], whole.pred[q]), q
    product = run(rv, fx, pairs="product")
    assert same(product.table(), whole.table()) and same(product.pred, whole.pred) and [tuple(p) for p in product.pairs] == fx.pairs
    perm = np.random.default_rng(5).permutation(len(fx.pairs))
    shuffled = run(rv, fx, pairs=[fx.pairs[k] for k in perm])
    assert same(shuffled.table(), whole.table()[perm]) and same(shuffled.pred, whole.pred[perm])


def test_a_recording_of_the_ragged_batch_equals_the_recording_alone(rv, gpu):
    for fx in (hr.fixture_b(5, 1), hr.fixture_b(5, 3, hr.EULER), hr.fixture_b(5, 1, hr.RK4, hr.PREV_INTERP, True)):
        whole = gpu(fx)
        for b, n in enumerate(fx.lengths):
            kw = dict(fx.kwargs(), lengths=None, return_pred=True)
            alone = rv.score_pairs(fx.theta_rows, fx.gamma_rows, fx.X[b, :n], fx.time[b, :n], fx.theta[b, :n], fx.gamma[b, :n], fx.mean, fx.scale, **kw)
            assert same(alone.table()[:, 0], whole.table()[:, b]), (fx.name, b)
            Wb = alone.pred.shape[2]
            assert Wb == hr.n_windows(n, fx.H, fx.stride) == whole.windows[b]
            assert same(alone.pred[:, 0], whole.pred[:, b, :Wb]) and np.isnan(whole.pred[:, b, Wb:]).all(), (fx.name, b)


def test_device_entry_gives_the_host_entry_bits(rv, gpu):
    for fx in (hr.fixture_b(5, 1), hr.fixture_b(1, 3), hr.fixture_b(5, 3, hr.EULER, hr.PREV_INTERP, True)):
        dev = run(rv, fx, device=True)
        assert same(dev.table(), gpu(fx).table()) and same(dev.pred, gpu(fx).pred), fx.name
    fx = hr.fixture_a()
    dev = run(rv, fx, device=True, return_pred=False)
    assert dev.pred is None and same(dev.table(), gpu(fx).table())


# ---- 6. edge shapes -------------------------------------------------------------------------------------------------------------------
def test_edge_shapes(rv, gpu):
    for H, stride in ((1, 1), (1, 3), (5, 1), (5, 3)):
        fx = hr.fixture_b(H, stride)
        sk = gpu(fx)
        assert list(sk.windows) == [hr.n_windows(n, H, stride) for n in fx.lengths]
        none = [b for b, n in enumerate(fx.lengths) if n <= H]             # len 1, and 2 and H where they are no more than H: no window
        assert fx.lengths[0] == 1 and 0 in none and len(none) == (3 if H == 5 else 2) and fx.lengths[3] == H + 1 and sk.windows[3] == 1
        t = sk.table()
        for b in none:
            assert (t[:, b, :, 4] == 0).all() and np.isnan(t[:, b][..., [0, 1, 2, 3, 5, 6, 7, 8]]).all() and np.isnan(sk.pred[:, b]).all()
            assert np.isnan(sk.coverage[:, b]).all() and np.isnan(sk.skill[:, b]).all()
        assert (t[:2, 3, :, 4] == 1).all() and np.isfinite(t[:2, 3]).all()
    # stride > H
    assert hr.fixture_b(1, 3).stride > hr.fixture_b(1, 3).H
    # log(x3): the pairs with it drop exactly the windows horizon_np drops, and a dropped window stays out
    fx = hr.fixture_b(5, 1)
    sk = gpu(fx)
    for q in (3, 6, 7):
        for b in (4, 5):
            ref = fx.np_pair(q, b)[0]
            assert (sk.n_ok[q, b] == ref[:, 4]).all(), (q, b)
            assert 0 < sk.n_ok[q, b, 0] < sk.windows[b] and (np.diff(sk.n_ok[q, b]) <= 0).all() and sk.n_ok[q, b, -1] < sk.n_ok[q, b, 0]
            bad = ~np.isfinite(sk.pred[q, b, :sk.windows[b], :, :]).all(axis=2)
            assert (np.maximum.accumulate(bad, axis=1).sum(axis=0) == sk.windows[b] - sk.n_ok[q, b]).all()
    without = run(rv, fx, pairs=[p for p in fx.pairs if 3 not in p])       # the other pairs are untouched by the bad ones
    keep = [q for q, p in enumerate(fx.pairs) if 3 not in p]
    assert same(without.table(), sk.table()[keep])
    # a non-finite truth takes a window out at that step only
    fx = hr.fixture_b(5, 3)
    theta = fx.theta.copy()
    theta[5, 9] = np.nan
    sk = rv.score_pairs(fx.theta_rows, fx.gamma_rows, fx.X, fx.time, theta, fx.gamma, fx.mean, fx.scale, **dict(fx.kwargs(), return_pred=True))
    ref = hr.skill_from_pred(sk.pred[0, 5], theta[5], fx.gamma[5], fx.lengths[5], 5, 3)
    assert same(sk.table()[0, 5][:, 2:], ref[:, 2:]) and ref[:, 4].min() < sk.windows[5]


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_launched(rv):
    from rovmpc import _lib, expr
    from rovmpc.engine import _ptr
    PUSH_F, PUSH_C, ADD = (expr.OP[n] for n in ("PUSH_F", "PUSH_C", "ADD"))
    T, B, F, H = 8, 2, 6, 3
    slots = (2, 3, 4, 5, -1, -1)
    front = dict(code=np.array([PUSH_F, (0 << 8) | PUSH_C, ADD, (1 << 8) | PUSH_F], np.int32), code_off=np.array([0, 3, 4], np.int32),
                 consts=np.array([0.5]), const_off=np.array([0, 1, 1], np.int32), R=2)
    good = dict(t=front, g=front, pairs=np.array([[0, 1], [1, 0], [1, 1]], np.int32), Q=3, X=np.zeros((B, T, F)), F=F, mean=np.zeros(F),
                scale=np.ones(F), time=np.tile(np.arange(T) * 0.1, (B, 1)), len=np.array([T, 5], np.int64), T=T, B=B,
                theta=np.zeros((B, T)), gamma=np.zeros((B, T)), params=_lib.HorizonParams.make(H, 1, slots=slots), skill=1, pred=1)
    e = rv.default_engine()
    p_ = lambda v: _ptr(v) if isinstance(v, np.ndarray) else v

    def call(**change):
        a = dict(good)
        for k, v in change.items():
            if k in ("t", "g"):
                a[k] = dict(front, **v)
            else:
                a[k] = v
        skill = np.full((max(a["Q"], 1), max(a["B"], 1), H, 9), -7.0)
        pred = np.full((max(a["Q"], 1), max(a["B"], 1), T, H, 2), -7.0)
        fr = lambda f: [p_(f["code"]), p_(f["code_off"]), p_(f["consts"]), p_(f["const_off"]), f["R"]]
        params = a["params"]
        rc = e.lib.rovmpc_score_pairs(e._h, *fr(a["t"]), *fr(a["g"]), p_(a["pairs"]), a["Q"], p_(a["X"]), a["F"], p_(a["mean"]), p_(a["scale"]),
                                      p_(a["time"]), p_(a["len"]), a["T"], a["B"], p_(a["theta"]), p_(a["gamma"]),
                                      None if params is None else C.byref(params), _ptr(skill) if a["skill"] is not None else None,
                                      _ptr(pred) if a["pred"] is not None else None)
        return rc, e.lib.rovmpc_last_error(e._h).decode(), skill, pred

    rc, _, skill, pred = call()
    assert rc == 0 and not (skill == -7.0).any()
    W = hr.n_windows(T, H, 1)
    assert not (pred.reshape(-1)[:3 * B * W * H * 2] == -7.0).any()
    rc, _, skill, _ = call(pred=None)
    assert rc == 0 and not (skill == -7.0).any()

    def params(**kw):
        p = _lib.HorizonParams.make(H, 1, slots=slots)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    wide = np.zeros((B, T, _lib.MAX_FEATURES + 1))
    bad = [dict(Q=0), dict(B=0), dict(T=0), dict(t=dict(R=0)), dict(g=dict(R=0)), dict(Q=(1 << 24) // B + 1), dict(F=0),
           dict(F=_lib.MAX_FEATURES + 1, X=wide), dict(params=params(H=0)), dict(params=params(stride=0)), dict(params=params(integrator=2)),
           dict(params=params(integrator=-1)), dict(params=params(prev_mode=2)), dict(pairs=np.array([[0, 2], [0, 0], [0, 0]], np.int32)),
           dict(pairs=np.array([[0, 0], [-1, 0], [0, 0]], np.int32)), dict(params=params(slot_theta=-1)), dict(params=params(slot_gamma=-1)),
           dict(params=params(slot_theta=F)), dict(params=params(slot_sin_gamma=-2)), dict(params=params(slot_cos_theta=2)),
           dict(params=params(slot_gamma_prev=4)), dict(scale=np.where(np.arange(F) == 3, 0.0, 1.0)), dict(scale=np.where(np.arange(F) == 5, np.inf, 1.0)),
           dict(scale=np.where(np.arange(F) == 2, np.nan, 1.0)), dict(mean=np.where(np.arange(F) == 4, np.nan, 0.0)),
           dict(t=dict(code_off=np.array([0, 4, 3], np.int32))), dict(g=dict(const_off=np.array([0, 1, 0], np.int32))),
           dict(g=dict(code_off=np.array([1, 3, 4], np.int32))), dict(len=np.array([T, 0], np.int64)), dict(len=np.array([T + 1, 1], np.int64)),
           dict(params=params(struct_size=40)), dict(t=dict(code=None)), dict(t=dict(code_off=None)), dict(t=dict(consts=None)),
           dict(g=dict(const_off=None)), dict(g=dict(code=None)), dict(pairs=None), dict(X=None), dict(mean=None), dict(scale=None), dict(time=None),
           dict(theta=None), dict(gamma=None), dict(skill=None)]
    for change in bad:
        rc, msg, skill, pred = call(**change)
        assert rc == -1 and "rovmpc_score_pairs" in msg, (change, rc, msg)
        assert (skill == -7.0).all() and (pred == -7.0).all(), change
    # a scale of zero at a slot no name points to is not refused
    assert call(scale=np.where(np.arange(F) == 0, 0.0, 1.0))[0] == 0
    # a bad row is named with its front: gamma row 1 reads feature 1, which F = 1 does not have (the slots then fall outside too,
    # so the map is checked with F = 2: theta at 0, gamma at 1, and a row that reads feature 2)
    two = _lib.HorizonParams.make(H, 1, slots=(0, 1, -1, -1, -1, -1))
    reads2 = dict(code=np.array([PUSH_F, (0 << 8) | PUSH_C, ADD, (2 << 8) | PUSH_F], np.int32))
    rc, msg, skill, _ = call(F=2, X=np.zeros((B, T, 2)), mean=np.zeros(2), scale=np.ones(2), params=two, g=reads2)
    assert rc == -1 and "gamma row 1" in msg and (skill == -7.0).all(), msg
    rc, msg, skill, _ = call(t=dict(code=np.array([ADD, PUSH_F, PUSH_F, PUSH_F], np.int32)))
    assert rc == -1 and "theta row 0" in msg and (skill == -7.0).all(), msg
    assert "second-order" in call(params=params(integrator=3))[1]
    assert e.lib.rovmpc_score_pairs(None, *[None] * 4, 1, *[None] * 4, 1, None, 1, None, 1, None, None, None, None, 1, 1, None, None, None, None, None) == -1
    # the device entry makes the same checks
    rc = e.lib.rovmpc_score_pairs_device(e._h, *[None] * 4, 1, *[None] * 4, 1, None, 1, None, 1, None, None, None, None, 1, 1, None, None, None, None, None)
    assert rc == -1 and "rovmpc_score_pairs_device" in e.lib.rovmpc_last_error(e._h).decode()
    d = _lib.HorizonParams()
    e.lib.rovmpc_default_horizon_params(C.byref(d))
    ref = _lib.HorizonParams.make()
    assert bytes(d) == bytes(ref)


# ---- 8. select_model -------------------------------------------------------------------------------------------------------------------
def test_select_model_with_a_horizon_returns_the_chosen_pair(rv, gpu):
    fx = hr.fixture_a()
    X_raw = fx.X[0] * fx.scale + fx.mean
    args = (fx.theta_rows, fx.gamma_rows, X_raw, fx.time[0], fx.theta[0], fx.gamma[0], fx.mean, fx.scale)
    model, s_th, s_ga, sk = rv.select_model(*args, horizon=8)
    dm = rv.default_model()
    assert (model.expr_theta, model.expr_gamma) == (dm.expr_theta, dm.expr_gamma)
    assert tuple(sk.pairs[sk.best()]) == fx.pairs[fx.chosen] and len(sk.pairs) == 16 and (sk.n_ok[sk.best()] == 192).all()
    whole = gpu(fx)
    assert whole.best() == fx.chosen
    assert list(whole.rank()[:5]) == list(rv.PairSkill.from_table(np.stack([fx.np_pair(q, 0)[0] for q in range(len(fx.pairs))])[:, None],
                                                                   fx.pairs, whole.expressions, whole.windows).rank()[:5])
    # without a horizon: the three values of before, the rows of the open-loop ranking
    plain = rv.select_model(*args)
    assert len(plain) == 3
    m3, p_th, p_ga = plain
    assert (m3.expr_theta, m3.expr_gamma) == (p_th.expressions[p_th.best()], p_ga.expressions[p_ga.best()])
    assert same(p_th.table(), s_th.table()) and same(p_ga.table(), s_ga.table())
    assert same(p_th.table(), rv.score_rows(fx.theta_rows, (X_raw - fx.mean) / fx.scale, fx.time[0], fx.theta[0]).table())
