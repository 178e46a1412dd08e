"""The tail of the single-problem step: every workgroup hands its best trajectory to the sweeping workgroup as
self-tagged granules (epoch << 32 | 32 payload bits), and the sweeper builds the record [J*, k*, u(3), (theta, gamma)_0..N]
from the winner's granules.

The expected record of every case comes from ``Engine.rollout_costs(state, U, return_traj=True)`` on the same inputs --
that launch writes every candidate's trajectory itself and hands nothing over in granules: k* = argmin(J) with NaN -> inf
(lowest index on ties), and the record's trajectory is that candidate's rows.  Records are compared as raw bytes.
Workgroups hold 16 candidates (candidates_per_block = 16), so candidate k belongs to workgroup k // 16.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CK = 16
K_TWO_ROUNDS = 16 * 257          # one more workgroup than the MI355X has CUs: the sweeper is the last block of a two-round grid


@pytest.fixture(scope="module")
def rv():
    import rovmpc
    return rovmpc


@pytest.fixture(scope="module")
def engines(rv):
    """One engine per (K, N, dtype), shared by the tests of this module."""
    cache = {}

    def get(K, N, dtype="f64"):
        key = (K, N, dtype)
        if key not in cache:
            cache[key] = rv.Engine(rv.MPCConfig(N=N, K=K, dtype=dtype, candidates_per_block=CK))
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


def expected_record(eng, state, U):
    J, traj = eng.rollout_costs(state, U, return_traj=True)
    J = np.where(np.isnan(J), np.inf, J.astype(np.float64))
    k = int(np.argmin(J))
    return np.concatenate([[J[k], float(k)], np.asarray(U[k, 0, :], np.float64), traj[k].astype(np.float64).ravel()]), k


def run_steps(eng, state, batches, order):
    """len(order) launches back to back on one stream, launch i on batches[order[i]]; the records, one row per launch."""
    import torch
    dev = torch.device("cuda", 0)
    tdt = torch.float64 if eng.cfg.dtype == "f64" else torch.float32
    d_state = torch.tensor(np.asarray(state, np.float64), device=dev)
    d_U = [torch.tensor(np.ascontiguousarray(U, eng.cfg.np_dtype), device=dev, dtype=tdt) for U in batches]
    d_res = torch.full((len(order), eng.result_len), float("nan"), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for i, b in enumerate(order):
        eng.step_device(d_state.data_ptr(), d_U[b].data_ptr(), d_res[i].data_ptr(), stream)
    torch.cuda.synchronize()
    eng.device_status()
    return d_res.cpu().numpy()


def same_bytes(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def winner_at(eng, state, U, pos):
    """U with its best candidate swapped to index pos (a candidate's cost does not depend on its index)."""
    _, k = expected_record(eng, state, U)
    U = U.copy()
    U[[k, pos]] = U[[pos, k]]
    return U


# ---- 1. the winner in every position -----------------------------------------------------------------------------------
POSITIONS = [
    # K, N, dtype, index of the winner
    (64, 20, "f64", 3), (64, 20, "f64", 16 * 3 + 9), (64, 20, "f64", 16 * 1 + 15),
    (64, 4, "f64", 0), (64, 4, "f64", 63), (64, 4, "f64", 16 * 2 + 7),
    (64, 20, "f32", 16 * 3 + 2),
    (K_TWO_ROUNDS, 20, "f64", 5), (K_TWO_ROUNDS, 20, "f64", 16 * 256 + 11), (K_TWO_ROUNDS, 20, "f64", 16 * 100 + 1),
    (K_TWO_ROUNDS, 4, "f64", 16 * 256),
    (4096, 20, "f64", 16 * 255 + 3), (4096, 20, "f64", 16 * 130 + 1),   # 256 workgroups: the most that one wave sweeps alone
    (16, 20, "f64", 6), (16, 4, "f64", 15),                 # the sweeper sweeps only itself
    (40, 20, "f64", 2), (40, 20, "f64", 32 + 7), (40, 4, "f64", 16 + 4),      # nvalid = 8 < CK in the last workgroup
]


@pytest.mark.parametrize("K,N,dtype,pos", POSITIONS)
def test_winner_in_every_position(rv, engines, K, N, dtype, pos):
    eng = engines(K, N, dtype)
    state, U = rv.synthetic_problem(K, N, seed=300 + N, dtype=eng.cfg.np_dtype)
    U = winner_at(eng, state, U, pos)
    exp, k = expected_record(eng, state, U)
    assert k == pos
    rec = run_steps(eng, state, [U], [0, 0])
    assert same_bytes(rec[0], exp) and same_bytes(rec[1], exp), (rec[0][:5], exp[:5])


# ---- 2. stale data must not be read ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(64, 4), (64, 20), (K_TWO_ROUNDS, 20)])
def test_consecutive_launches_read_their_own_epoch(rv, engines, K, N):
    """One handle, 64 launches back to back cycling four candidate batches whose winners sit in different workgroups: a
    tag check that takes the previous launch's granules, or a winner guessed early and not corrected, shows as another
    batch's record."""
    eng = engines(K, N)
    nb = K // CK
    state, _ = rv.synthetic_problem(K, N, seed=41)
    batches, exps = [], []
    for i, wg in enumerate((0, nb - 1, nb // 2, 1)):
        U = winner_at(eng, state, rv.synthetic_problem(K, N, seed=410 + i)[1], CK * wg + (5 * i) % CK)
        exp, k = expected_record(eng, state, U)
        assert k // CK == wg
        batches.append(U); exps.append(exp)
    assert len({e.tobytes() for e in exps}) == 4
    order = [i % 4 for i in range(64)]
    rec = run_steps(eng, state, batches, order)
    for i, b in enumerate(order):
        assert same_bytes(rec[i], exps[b]), (i, b, rec[i][:2], exps[b][:2])


# ---- 3. the winner publishes last --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,wg", [(64, 20, 2), (64, 4, 0), (K_TWO_ROUNDS, 20, 130), (K_TWO_ROUNDS, 20, 256)])
def test_winner_in_the_slowest_workgroup(rv, engines, K, N, wg):
    """One candidate of workgroup wg carries a control of 3e10 mm/s, which puts that workgroup alone on the range-checked
    sine and the re-anchoring path, so it publishes behind the others; another candidate of the SAME workgroup is the
    global best.  Whatever the sweeper held for the winner before that workgroup published is wrong.  (Passing does not
    depend on the timing; the timing only makes it hard.)"""
    eng = engines(K, N)
    state, U = rv.synthetic_problem(K, N, seed=77)
    U = winner_at(eng, state, U, CK * wg + 5)
    U[CK * wg + 0, N // 2, 0] = 3e10
    exp, k = expected_record(eng, state, U)
    assert k == CK * wg + 5
    rec = run_steps(eng, state, [U], [0, 0, 0])
    for r in rec:
        assert same_bytes(r, exp), (r[:5], exp[:5])


# ---- 4. bit patterns ---------------------------------------------------------------------------------------------------
def test_nan_payload_and_all_costs_nan(rv, engines):
    """theta_0 = a NaN with its own payload (not the theta-slot marker 0x7ff85ea71e5007e7): every cost is NaN, so
    J* = inf and k* = 0, and the record's trajectory carries candidate 0's bytes untouched."""
    K, N = 64, 20
    eng = engines(K, N)
    state, U = rv.synthetic_problem(K, N, seed=5)
    state = np.asarray(state, np.float64).copy()
    state[12] = np.array([0x7ff8000000abcdef], dtype=np.uint64).view(np.float64)[0]
    exp, k = expected_record(eng, state, U)
    assert k == 0 and exp[0] == np.inf
    rec = run_steps(eng, state, [U], [0, 0])
    assert rec[0][0] == np.inf and rec[0][1] == 0.0
    assert same_bytes(rec[0], exp) and same_bytes(rec[1], exp)


@pytest.mark.parametrize("N", [4, 20])
def test_negative_zero_gamma(rv, engines, N):
    K = 64
    eng = engines(K, N)
    state, U = rv.synthetic_problem(K, N, seed=6)
    state = np.asarray(state, np.float64).copy()
    state[13] = -0.0
    U = winner_at(eng, state, U, 16 * 3 + 1)
    exp, _ = expected_record(eng, state, U)
    rec = run_steps(eng, state, [U], [0])
    assert same_bytes(rec[0], exp)
    assert np.signbit(rec[0][6]) and rec[0][6] == 0.0          # gamma_0 = -0.0 came through


# ---- 5. ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,lo,hi", [(64, 20, 16 * 0 + 9, 16 * 3 + 2), (64, 4, 16 * 1 + 15, 16 * 2 + 0),
                                       (K_TWO_ROUNDS, 20, 16 * 7 + 3, 16 * 256 + 3)])
def test_tie_goes_to_the_lower_index(rv, engines, K, N, lo, hi):
    eng = engines(K, N)
    state, U = rv.synthetic_problem(K, N, seed=8)
    for first in (lo, hi):                       # the original at either end, its copy at the other
        V = winner_at(eng, state, U, first)
        V[lo + hi - first] = V[first]
        exp, k = expected_record(eng, state, V)
        assert k == lo
        rec = run_steps(eng, state, [V], [0, 0])
        assert same_bytes(rec[0], exp) and same_bytes(rec[1], exp), (rec[0][:2], exp[:2])


# ---- 6. batched --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 20])
def test_batched_records_equal_single_launches(rv, engines, N):
    import torch
    B, K = 3, 64
    eng = engines(K, N)
    dev = torch.device("cuda", 0)
    states = np.empty((B, 16)); U = np.empty((B, K, N, 3))
    for b in range(B):
        states[b], U[b] = rv.synthetic_problem(K, N, seed=600 + b)
        states[b, 12:14] += 0.01 * b
        U[b] = winner_at(eng, states[b], U[b], 16 * (3 - b) + b)      # winners in workgroups 3, 2, 1
    d_states = torch.tensor(states, device=dev); d_U = torch.tensor(U, device=dev)
    d_res = torch.full((B, eng.result_len), float("nan"), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        eng.step_batch_device(B, d_states.data_ptr(), d_U.data_ptr(), d_res.data_ptr(), stream)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy()
    for b in range(B):
        exp, k = expected_record(eng, states[b], U[b])
        assert k == 16 * (3 - b) + b
        single = run_steps(eng, states[b], [U[b]], [0])[0]
        assert same_bytes(res[b], single), b
        assert same_bytes(res[b], exp), b
