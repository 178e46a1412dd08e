"""The options of one rollout launch -- cost destination, mailbox, slot hand-off flags, fused plant update, batch size -- belong
to that launch alone.  One handle runs the entry points that set them one after the other (a batched step, MPPI, the sampled
step, each closed-loop form, the all-reduce step with a slot reused); a plain rovmpc_step_device between them, every loop and
every sampled step must give the records of a fresh handle that runs nothing else, and rovmpc_batch_costs_device must go on
naming the batched launch's costs.  Compiled-in model and a hiprtc model (whose sampled step is the stand-alone sampler plus a
rollout with a mailbox, and whose loops launch the module's two entries).  Comparisons are of bit patterns: no tolerance."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plan_controller_helpers import defaults, rv  # noqa: E402,F401

pytestmark = pytest.mark.gpu

N, K, T = 12, 256, 3


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def loop_records(rep):
    return np.column_stack([rep.cost, rep.index.astype(np.float64), rep.u, rep.theta_gamma[1:]])


@pytest.mark.parametrize("rows,path", [(None, "builtin"), ((5, 9), "jit")], ids=["builtin", "jit"])
def test_a_launch_leaves_nothing_behind_for_the_next(rv, rows, path):
    import torch
    from rovmpc.closed_loop import closed_loop_pools, run_closed_loop
    from rovmpc.sharded import NativeShardedMPC
    dev = torch.device("cuda", 0)
    hip = ctypes.CDLL("libamdhip64.so")
    model = rv.default_model(*rows) if rows else None
    mean, std = defaults(rv, N)
    state, U = rv.synthetic_problem(K, N)
    d_state, d_U = torch.tensor(state, device=dev), torch.tensor(U, device=dev)
    mp = rv.MPPIParams.make(2, 0.5, std)

    def engine():
        e = rv.Engine(rv.MPCConfig(N=N, K=K), model)
        assert e.model_path == path
        e.set_option("handoff_timeout_ms", 2000.0)          # a regression fails in seconds
        return e

    def plain_step(e):
        rec = torch.zeros(e.result_len, dtype=torch.float64, device=dev)
        e.step_device(d_state.data_ptr(), d_U.data_ptr(), rec.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rec.cpu().numpy()

    def sampled(e):
        return [e.mpc_step_sampled(state, 42, s, mean[0], std, True).copy() for s in range(2)]

    def loop(e, mode=""):
        return loop_records(run_closed_loop(e, 12, T, feedback=True, mode=mode, pools=pools))

    def batch_costs(e):
        J = torch.empty(2 * K, dtype=torch.float64, device=dev)
        ptr = e.batch_costs_ptr()
        assert hip.hipMemcpy(ctypes.c_void_p(J.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(2 * K * 8), 3) == 0
        return ptr, J.cpu().numpy()

    # what a fresh handle gives for each call on its own
    with engine() as f:
        pools = closed_loop_pools(f, 8, 3)                   # (the sampler only: no rollout launch)
        want_step = plain_step(f)
    with engine() as f:
        want_sampled = sampled(f)
    with engine() as f:
        want_per_step = loop(f)
        assert f.closed_loop_form == "per_step"
    with engine() as f:
        want_pipelined = loop(f, "pipelined")
        assert f.closed_loop_form == "pipelined"
    with engine() as f:
        smpc = NativeShardedMPC(f, rank=0, world=1)
        try:
            want_handoff = loop(f)
            assert f.closed_loop_form == "sharded_handoff"
        finally:
            smpc.close()
    assert np.isfinite(want_step[0]) and all(np.isfinite(w[:, 0]).all() for w in (want_per_step, want_pipelined, want_handoff))

    with engine() as a:
        # 1. a batched launch: rovmpc_batch_costs_device names its costs
        d_states2 = torch.tensor(np.tile(state, (2, 1)), device=dev)
        d_U2 = torch.tensor(np.stack([U, U * 1.01]), device=dev)
        d_res2 = torch.zeros((2, a.result_len), dtype=torch.float64, device=dev)
        a.step_batch_device(2, d_states2.data_ptr(), d_U2.data_ptr(), d_res2.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ptr1, J1 = batch_costs(a)
        assert np.isfinite(J1).any() and not same(J1[:K], J1[K:])
        # 2. MPPI writes its own costs: the batched launch's stay where and what they were
        a.mppi_reset(mean)
        a.mppi_step(state, 3, 0, mp)
        ptr2, J2 = batch_costs(a)
        assert ptr2 == ptr1 and same(J2, J1)
        # 3. the sampled step (a mailbox)
        got_sampled = sampled(a)
        assert all(same(x, y) for x, y in zip(got_sampled, want_sampled))
        # 4. a plain step
        assert same(plain_step(a), want_step)                                        # r1
        # 5. launch per step with the plant update fused into the step
        assert same(loop(a), want_per_step) and a.closed_loop_form == "per_step"
        assert same(plain_step(a), want_step)                                        # r2
        # 6. pipelined
        assert same(loop(a, "pipelined"), want_pipelined) and a.closed_loop_form == "pipelined"
        assert same(plain_step(a), want_step)                                        # r3
        # 7. the all-reduce step, one more than the slots, then the GPU-side hand-off loop on the same slots
        smpc = NativeShardedMPC(a, rank=0, world=1)
        try:
            recs = torch.zeros((5, a.result_len), dtype=torch.float64, device=dev)
            for i in range(5):
                a.step_device_allreduce(d_state.data_ptr(), d_U.data_ptr(), 0, recs[i].data_ptr(), torch.cuda.current_stream().cuda_stream)
            smpc.synchronize()
            torch.cuda.synchronize()
            for r in recs.cpu().numpy():
                assert same(r[:5], want_step[:5])                                    # cost, index, control
            assert same(loop(a), want_handoff) and a.closed_loop_form == "sharded_handoff"
            assert same(plain_step(a), want_step)                                    # r4
        finally:
            smpc.close()
        a.device_status()
