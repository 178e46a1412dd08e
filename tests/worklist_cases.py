"""Cases of tests/golden/rollout_worklists.npz: the smallest launches at which the partition of the per-node geometry
(phase 4a / 4b items) over the waves of a rollout workgroup can go wrong.  Shared by tools/make_worklist_golden.py, which
records the bytes, and tests/test_worklist_balance_gpu.py, which holds every later build to them."""
import ctypes
import os
from collections import namedtuple

import numpy as np

K = 40            # 16 candidates per workgroup: two full workgroups and one with 8 valid candidates
CK = 16

Case = namedtuple("Case", "name N NT dtype no_builtin hold")
CASES = (
    Case("n20_nt320", 20, 320, "f64", False, False),          # the headline instance: 320 items, early batch of 64
    Case("n20_nt256", 20, 256, "f64", False, False),          # early batch of 64 beside a pool of 192 threads
    Case("n20_nt512", 20, 512, "f64", False, False),          # more pool threads than items: idle waves
    Case("n20_nt192", 20, 192, "f64", False, False),          # the smallest workgroup that still has an early batch
    Case("n17_nt320", 17, 320, "f64", False, False),          # 272 items: early batch of 16, a partial early wave
    Case("n24_nt448", 24, 448, "f64", False, False),          # 384 items: no early batch
    Case("n36_nt512", 36, 512, "f64", False, False),          # 576 items: early batch of 64, two rounds after the join
    Case("n20_nt320_f32", 20, 320, "f32", False, False),
    Case("n20_nt320_jit", 20, 320, "f64", True, False),       # the default model through the hiprtc route
    Case("n20_nt320_hold", 20, 320, "f64", False, True),      # HOLD delay mode: the theta loop with run-time flags
)
LITERAL = (("literal_n", False), ("runtime_n", True))        # ROVMPC_NO_LITERAL_N unset / set


def run_case(rv, case, no_literal_n):
    """{part: array} of one case: the record of rovmpc_step, J[K] of rovmpc_rollout_costs, and the record and
    rovmpc_batch_costs_device's J[K] of a one-problem rovmpc_step_batch_device."""
    import torch
    saved = os.environ.pop("ROVMPC_NO_LITERAL_N", None)
    if no_literal_n:
        os.environ["ROVMPC_NO_LITERAL_N"] = "1"
    try:
        cfg = rv.MPCConfig(N=case.N, K=K, dtype=case.dtype, candidates_per_block=CK, threads_per_block=case.NT,
                           no_builtin=case.no_builtin, prev_mode=rv.PREV_HOLD if case.hold else rv.PREV_INTERP, debug_flags=0)
        state, U = rv.synthetic_problem(K, case.N, seed=4100 + case.N, dtype=cfg.np_dtype)
        dev = torch.device("cuda", 0)
        out = {}
        with rv.Engine(cfg) as e:
            assert (e.model_path == "jit") == case.no_builtin, e.model_path
            r = e.step(state, U)
            out["step_record"] = np.concatenate([[r.cost, float(r.index)], r.u, r.traj.reshape(-1)])
            out["costs_J"] = e.rollout_costs(state, U)
            d_s, d_U = torch.tensor(state[None], device=dev), torch.tensor(U[None], device=dev)
            d_r = torch.full((1, e.result_len), float("nan"), dtype=torch.float64, device=dev)
            e.step_batch_device(1, d_s.data_ptr(), d_U.data_ptr(), d_r.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            d_J = torch.empty(K, dtype=d_U.dtype, device=dev)
            rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(d_J.data_ptr()), ctypes.c_void_p(e.batch_costs_ptr()),
                                                         ctypes.c_size_t(K * d_J.element_size()), 3)      # device to device
            assert rc == 0, rc
            out["batch_record"] = d_r.cpu().numpy()[0]
            out["batch_J"] = d_J.cpu().numpy()
        return out
    finally:
        os.environ.pop("ROVMPC_NO_LITERAL_N", None)
        if saved is not None:
            os.environ["ROVMPC_NO_LITERAL_N"] = saved
