"""Cases of tests/golden/rollout_prologue.npz: the smallest launches at which the rollout kernel's prologue can go wrong --
the copy of the candidate controls into LDS (phase 0) and the set-up the gamma and theta waves do before their chains.
Shared by tools/make_prologue_golden.py, which records the bytes, and tests/test_rollout_prologue_gpu.py, which holds every
later build to them.

Control copy: 19 candidates are one full workgroup of 16 and one with 3 valid candidates, 40 are two full ones and one with
8.  A row of N = 7 steps is 21 elements, so the 16-byte chunks of the copy straddle candidates; N = 1 is a 3-element row.
The candidate tensor is handed over three ways: compact (16-byte aligned), as a view one element into a larger buffer (the
unaligned path), and as an aligned view whose neighbours on both sides are NaN (a load outside [U, U + K 3 N) would show in
the record as a NaN or a changed arg-min only by luck -- the padding rows of the last workgroup are where it would land --
so the test also compares the record with the compact run's)."""
import ctypes
import os
from collections import namedtuple

import numpy as np

CK = 16
LAYOUTS = ("compact", "offset1", "fenced")

Copy = namedtuple("Copy", "name K N NT dtype")
COPY_CASES = tuple(
    Copy(f"k{K}_n{N}_nt{NT}_{dt}", K, N, NT, dt)
    for dt in ("f64", "f32")
    for K, N, NT in ((19, 1, 320), (19, 7, 320), (19, 20, 320), (40, 1, 64), (40, 7, 128), (40, 20, 512),
                     (19, 7, 64), (40, 20, 128), (19, 20, 512), (40, 7, 320))
)

Setup = namedtuple("Setup", "name theta0 integrator hold vt")
BIG_THETA = float(2 ** 26) * 1.5 + 0.3          # beyond the fast reduction of the sine: the out-of-line one
SETUP_CASES = (
    Setup("theta06", 0.6, "rk4", False, 1),
    Setup("theta15", 1.5, "rk4", False, 1),
    Setup("theta_big", BIG_THETA, "rk4", False, 1),
    Setup("theta_nan", float("nan"), "rk4", False, 1),
    Setup("euler", 0.6, "euler", False, 1),          # Euler and HOLD take the theta loop with run-time flags
    Setup("hold", 0.6, "rk4", True, 1),
    Setup("euler_theta15", 1.5, "euler", False, 1),
    Setup("vt_none", 1.5, "rk4", False, 0),
    Setup("vt_table", 1.5, "rk4", False, 2),
    Setup("vt_none_hold", 0.6, "rk4", True, 0),
)
LITERAL = (("literal_n", False), ("runtime_n", True))        # ROVMPC_NO_LITERAL_N unset / set
SETUP_K, SETUP_N, SETUP_NT = 40, 20, 320

LOOP_K, LOOP_N, LOOP_STEPS, LOOP_POOLS = 256, 20, 50, 4


class literal_n:
    """ROVMPC_NO_LITERAL_N set or unset for the engines created inside the block."""

    def __init__(self, no_literal_n):
        self.no = no_literal_n

    def __enter__(self):
        self.saved = os.environ.pop("ROVMPC_NO_LITERAL_N", None)
        if self.no:
            os.environ["ROVMPC_NO_LITERAL_N"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("ROVMPC_NO_LITERAL_N", None)
        if self.saved is not None:
            os.environ["ROVMPC_NO_LITERAL_N"] = self.saved


def _place(U, layout, dev):
    """(tensor that owns the memory, view of it holding U) for one of LAYOUTS."""
    import torch
    flat = torch.tensor(np.ascontiguousarray(U).reshape(-1), device=dev)
    per16 = 16 // flat.element_size()
    if layout == "compact":
        assert flat.data_ptr() % 16 == 0
        return flat, flat
    lead = 1 if layout == "offset1" else 8 * per16
    fill = 0.0 if layout == "offset1" else float("nan")
    buf = torch.full((lead + flat.numel() + 8 * per16,), fill, dtype=flat.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + flat.numel()]
    view.copy_(flat)
    assert (view.data_ptr() % 16 != 0) == (layout == "offset1")
    return buf, view


def _batch_J(e, B, K, tdt, dev):
    import torch
    d_J = torch.empty(B * K, dtype=tdt, device=dev)
    rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(d_J.data_ptr()), ctypes.c_void_p(e.batch_costs_ptr()),
                                                 ctypes.c_size_t(d_J.numel() * d_J.element_size()), 3)      # device to device
    assert rc == 0, rc
    return d_J.cpu().numpy()


def run_copy_case(rv, case):
    """{layout/part: array}: the record of rovmpc_step_device and, from a one-problem rovmpc_step_batch_device on the same
    view, its record and J[K]."""
    import torch
    dev = torch.device("cuda", 0)
    cfg = rv.MPCConfig(N=case.N, K=case.K, dtype=case.dtype, candidates_per_block=CK, threads_per_block=case.NT)
    state, U = rv.synthetic_problem(case.K, case.N, seed=5200 + 10 * case.N + case.K, dtype=cfg.np_dtype)
    tdt = torch.float64 if case.dtype == "f64" else torch.float32
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    with rv.Engine(cfg) as e:
        d_s = torch.tensor(state[None], device=dev)
        for layout in LAYOUTS:
            own, view = _place(U, layout, dev)
            d_r = torch.full((2, e.result_len), float("nan"), dtype=torch.float64, device=dev)
            e.step_device(d_s.data_ptr(), view.data_ptr(), d_r[0].data_ptr(), stream)
            e.step_batch_device(1, d_s.data_ptr(), view.data_ptr(), d_r[1].data_ptr(), stream)
            torch.cuda.synchronize()
            e.device_status()
            out[f"{layout}/step_record"] = d_r[0].cpu().numpy()
            out[f"{layout}/batch_record"] = d_r[1].cpu().numpy()
            out[f"{layout}/batch_J"] = _batch_J(e, 1, case.K, tdt, dev)
            del own
    return out


def run_batch_case(rv):
    """B = 3 problems in one launch (K = 19, N = 7, fp64), the candidates of all three in one unaligned view."""
    import torch
    B, K, N = 3, 19, 7
    dev = torch.device("cuda", 0)
    cfg = rv.MPCConfig(N=N, K=K, candidates_per_block=CK, threads_per_block=320)
    states = np.empty((B, 16)); U = np.empty((B, K, N, 3))
    for b in range(B):
        states[b], U[b] = rv.synthetic_problem(K, N, seed=5300 + b)
        states[b, 12:14] += 0.01 * b
    out = {}
    with rv.Engine(cfg) as e:
        d_s = torch.tensor(states, device=dev)
        for layout in LAYOUTS:
            own, view = _place(U, layout, dev)
            d_r = torch.full((B, e.result_len), float("nan"), dtype=torch.float64, device=dev)
            e.step_batch_device(B, d_s.data_ptr(), view.data_ptr(), d_r.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            e.device_status()
            out[f"{layout}/batch_record"] = d_r.cpu().numpy()
            out[f"{layout}/batch_J"] = _batch_J(e, B, K, torch.float64, dev)
            del own
    return out


def run_sampled_case(rv):
    """Two sampled steps at one seed (K = 40, N = 20 and K = 19, N = 7): the controls are drawn in phase 0."""
    out = {}
    m = rv.default_model()
    for K, N in ((40, 20), (19, 7)):
        state, _ = rv.synthetic_problem(K, N, seed=5400 + N)
        with rv.Engine(rv.MPCConfig(N=N, K=K, candidates_per_block=CK, threads_per_block=320)) as e:
            recs = [e.mpc_step_sampled(state, 77, s, m.mean[3:6], m.scale[3:6]).copy() for s in range(2)]
        out[f"k{K}_n{N}/records"] = np.stack(recs)
    return out


def rand_rtab(N, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        out.append(q)
    return np.stack(out)


def run_setup_case(rv, case, no_literal_n):
    """{part: array}: record of rovmpc_step, J[K] and every candidate's trajectory of rovmpc_rollout_costs."""
    with literal_n(no_literal_n):
        cfg = rv.MPCConfig(N=SETUP_N, K=SETUP_K, candidates_per_block=CK, threads_per_block=SETUP_NT, vt_mode=case.vt,
                           integrator=rv.EULER if case.integrator == "euler" else rv.RK4,
                           prev_mode=rv.PREV_HOLD if case.hold else rv.PREV_INTERP)
        state, U = rv.synthetic_problem(SETUP_K, SETUP_N, seed=5500)
        state = np.asarray(state, np.float64).copy()
        state[12] = case.theta0
        state[14] = case.theta0 - 0.001
        with rv.Engine(cfg) as e:
            if case.vt == 2:
                e.set_rotation_table(rand_rtab(SETUP_N))
            r = e.step(state, U)
            J, traj = e.rollout_costs(state, U, return_traj=True)
        return {"step_record": np.concatenate([[r.cost, float(r.index)], r.u, r.traj.reshape(-1)]), "costs_J": J, "traj": traj}


def run_loop_case(rv):
    """50 steps of the pipelined closed loop with the model's own (theta, gamma) fed back: the records."""
    import torch
    from rovmpc.closed_loop import closed_loop_inputs, velocity_prior
    dev = torch.device("cuda", 0)
    with rv.Engine(rv.MPCConfig(N=LOOP_N, K=LOOP_K)) as e:
        e.set_option("handoff_timeout_ms", 2000.0)
        rows, state = closed_loop_inputs(e, 12, LOOP_STEPS, 0)
        vm, vs = velocity_prior(e)
        pools = vm + vs * np.random.default_rng(5600).standard_normal((LOOP_POOLS, LOOP_K, LOOP_N, 3))
        d_pools = torch.tensor(pools, device=dev); d_exo = torch.tensor(rows, device=dev); d_state = torch.tensor(state, device=dev)
        d_res = torch.full((LOOP_STEPS, e.result_len), float("nan"), dtype=torch.float64, device=dev)
        e.closed_loop_device(d_exo.data_ptr(), LOOP_STEPS, d_state.data_ptr(), d_pools.data_ptr(), LOOP_POOLS, d_res.data_ptr(),
                             0, True, torch.cuda.current_stream().cuda_stream, mode="pipelined")
        torch.cuda.synchronize()
        e.device_status()
        assert e.closed_loop_form == "pipelined"
        return {"records": d_res.cpu().numpy()}


def all_cases(rv):
    """(key prefix, thunk) of every recorded case, in the fixture's order."""
    for c in COPY_CASES:
        yield f"copy/{c.name}", (lambda c=c: run_copy_case(rv, c))
    yield "batch3", (lambda: run_batch_case(rv))
    yield "sampled", (lambda: run_sampled_case(rv))
    for c in SETUP_CASES:
        for tag, no in LITERAL:
            yield f"setup/{c.name}/{tag}", (lambda c=c, no=no: run_setup_case(rv, c, no))
    yield "loop", (lambda: run_loop_case(rv))
