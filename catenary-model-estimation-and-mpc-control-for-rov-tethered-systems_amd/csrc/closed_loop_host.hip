// closed_loop_host.hip -- the closed loop with the state handed over on the GPU: pipelined and sharded forms.
#include "rovmpc_internal.h"

#include "closed_loop_kernels.h"

// ---- closed loop ----------------------------------------------------------------------------------

// Workspace of the GPU-side closed-loop hand-off; fills the pointers of `p` and zeroes the sequence words on `s`.
static int closed_loop_workspace(rovmpc_handle *h, HandoffArgs &p, hipStream_t s) {
    const rovmpc_config &c = h->cfg;
    const size_t max_blocks = c.candidates_per_block > 0 ? (size_t)((c.K + c.candidates_per_block - 1) / c.candidates_per_block) : (size_t)c.K;
    if (!h->d_step_seq) {
        HIPCHK(h, hipMalloc((void **)&h->d_step_seq, 256));
        HIPCHK(h, hipMalloc((void **)&h->d_cl_granules, 2 * gran_stride((int)max_blocks, c.N) * sizeof(unsigned long long)));
        HIPCHK(h, hipMemset(h->d_cl_granules, 0, 2 * gran_stride((int)max_blocks, c.N) * sizeof(unsigned long long)));
        HIPCHK(h, hipMalloc((void **)&h->d_cl_blk_traj, 2 * max_blocks * (size_t)(c.N + 1) * 2 * sizeof(double)));
    }
    HIPCHK(h, hipMemsetAsync(h->d_step_seq, 0, 128, s));
    // the ring holds NaN until a step writes it: a wait that gives up before its state arrives reads NaN, not a state
    HIPCHK(h, hipMemsetAsync(h->d_step_seq + 16, 0xff, 128, s));
    p.seq_theta = h->d_step_seq; p.seq_gamma = h->d_step_seq + 8;             // separate 64-byte lines
    p.ring = reinterpret_cast<double *>(h->d_step_seq + 16);                   // [4][4] doubles
    p.granules2 = h->d_cl_granules; p.blk_traj2 = h->d_cl_blk_traj;
    return ROVMPC_OK;
}

// Resolves the closed-loop step kernel for geometry g into k (setting its dynamic-LDS attribute, as the launches need) and
// returns the workgroups of it the device holds at once: resident workgroups per CU x CUs; 0 if the model has no step kernel or
// a query fails (*why: that query's error).
static int step_kernel_capacity(rovmpc_handle *h, const Geo &g, Launchable &k, hipError_t *why = nullptr) {
    int capacity = 0;
    hipError_t e = rollout_launchable(h, LAUNCH_STEP, g, StepOpts(), k);
    if (e == hipSuccess) e = launchable_capacity(h, k, g.NT, &capacity);
    if (why) *why = e;
    return capacity;
}

// ---- pipelined closed loop: one step per launch, launches alternating between two streams -----------------------
template <typename T>
static int closed_loop_pipelined_t(rovmpc_handle *h, const double *d_exo, int64_t T_steps, double *d_state, const void *d_pools,
                                   int32_t n_pools, int32_t feedback, double *d_results, hipStream_t s) {
    Geo g = launch_geometry(h, 1);
    // Two launches are in flight at any time (launch g + 1 may start once launch g - 1 is complete), and the later one's
    // workgroups hold their CU slots while they wait for the earlier one's sweeper: both grids must fit the chip at once,
    // whatever order the two queues dispatch in.  Four-wave workgroups share a CU three at a time (measured with the HW_ID
    // stamp), five-wave ones do not: unless the caller fixed the geometry, use 256 threads.
    if (h->cfg.threads_per_block == 0 && h->cfg.candidates_per_block == 0 && g.NT > 256 && g.CK <= 16) g.NT = 256;
    // The launches alternate between the caller's stream and the process's high-priority stream (process_pipe_stream):
    // streams of equal priority can share a hardware queue, and then nothing overlaps.
    if (!h->pipe_streams[1]) FAIL(h, ROVMPC_ERR_HIP, "no second stream for the pipelined closed loop");
    if (!h->pipe_placed) {
        // ... provided that stream does not sit on the caller's command-processor pipe (31 us per step instead of 15,
        // measured in round 2 with a stream created late): probe it, and others if it fails (choose_side_streams)
        h->pipe_placed = true;
        const char *e = getenv("ROVMPC_COMM_PLACE");
        if (!(e && !strcmp(e, "0"))) {
            std::vector<hipStream_t> chosen;
            int rc = choose_side_streams(h, s, {h->pipe_streams[1]}, 1, chosen, h->pipe_placement);
            if (rc) return rc;
            if (!chosen.empty() && chosen[0] != h->pipe_streams[1]) { h->pipe_streams[1] = chosen[0]; h->pipe_stream_owned = true; }
            if (getenv("ROVMPC_COMM_PLACE_VERBOSE")) fprintf(stderr, "[rovmpc] pipelined loop's second stream: %s\n", h->pipe_placement.c_str());
        }
    }
    if (!h->pipe_ev[0])
        for (auto &ev : h->pipe_ev) HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const size_t R = rovmpc_result_len(h);
    RolloutArgs<T> a;
    HandoffArgs p;
    int rcw = closed_loop_workspace(h, p, s);
    if (rcw) return rcw;
    p.T = T_steps; p.exo = d_exo;
    const size_t pool_bytes = (size_t)h->cfg.K * h->cfg.N * 3 * sizeof(T);
    if (h->model_kind == MODEL_JIT && !h->jit_fn_step) FAIL(h, ROVMPC_ERR_UNSUPPORTED, "the run-time specialised module has no pipelined entry");
    if (h->model_kind == MODEL_INTERP)
        FAIL(h, ROVMPC_ERR_UNSUPPORTED, "pipelined closed loop: compiled-in and hiprtc-specialised models only (the interpreter runs launch per step)");
    Launchable k;
    hipError_t e;
    const int capacity = step_kernel_capacity(h, g, k, &e);
    if (e != hipSuccess && !k.mod) FAIL(h, ROVMPC_ERR_HIP, "occupancy query failed: %s", hipGetErrorString(e));      // (a module's failed query: capacity 0)
    if (2 * g.nblocks > capacity)
        FAIL(h, ROVMPC_ERR_UNSUPPORTED, "pipelined closed loop needs two grids resident at once: 2 x %d workgroups exceed the device's capacity %d "
                                        "(use rovmpc_closed_loop_device)", g.nblocks, capacity);
    h->cl_form = 2;
    hipLaunchKernelGGL(plant_update_kernel, dim3(1), dim3(64), 0, s, d_state, d_exo, (const double *)nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->pipe_ev[2], s));
    HIPCHK(h, hipStreamWaitEvent(h->pipe_streams[1], h->pipe_ev[2], 0));
    StepOpts o;
    o.plant_feedback = feedback ? 1 : 0;
    for (int64_t i = 0; i < T_steps; ++i) {
        hipStream_t st = (i & 1) ? h->pipe_streams[1] : s;
        fill_args<T>(h, a, d_state, (const char *)d_pools + (size_t)(i % n_pools) * pool_bytes, d_results + (size_t)i * R, g, o);
        a.sweeper = 0;
        p.step = i;
        e = launch_rollout<T>(h, k, a, 1, st, &p);                                                           // one epoch per step
        if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "pipelined closed-loop launch failed: %s", hipGetErrorString(e));
    }
    HIPCHK(h, hipEventRecord(h->pipe_ev[1], h->pipe_streams[1]));
    HIPCHK(h, hipStreamWaitEvent(s, h->pipe_ev[1], 0));
    return ROVMPC_OK;
}

// ---- sharded closed loop with the state handed over on the GPU ----------------------------------------------------------
// BASELINE config 5 as it is asked (every step the candidate-sharded one), model feedback: step g + 1's rollout is launched
// right behind step g's on the caller's stream -- no join, no plant-update kernel, no event on that stream -- and waits ON THE
// GPU for the state: gamma early from its own rank's sweeper (gamma's path is candidate-invariant, hence the same on every
// rank), theta from the select kernel that follows step g's all-reduce on the collective stream (the GLOBAL winner's first
// node).  Its controls load, positions, gamma table and first velocity-transform half run meanwhile, so a step costs
// rollout + max(0, all-reduce + select - prologue) instead of rollout + all-reduce + select + join + update
// (world 1: 47.5 -> ~20 us).  Compiled-in and hiprtc models whose step-kernel grid is resident in one round (the caller,
// rovmpc_closed_loop_device, checks that); records are the join-based loop's bit for bit.
template <typename T>
static int closed_loop_sharded_handoff_t(rovmpc_handle *h, const Launchable &k, const double *d_exo, int64_t T_steps, double *d_state,
                                         const void *d_pools, int32_t n_pools, int64_t k_offset, double *d_results, hipStream_t s) {
    const Geo g = launch_geometry(h, 1);
    const size_t R = rovmpc_result_len(h);
    if (!h->comm_placed) {
        int rc = place_comm_streams(h, s);
        if (rc) return rc;
    }
    HandoffArgs p;
    int rcw = closed_loop_workspace(h, p, s);
    if (rcw) return rcw;
    p.T = T_steps; p.exo = d_exo;
    const size_t pool_bytes = (size_t)h->cfg.K * h->cfg.N * 3 * sizeof(T);
    RolloutArgs<T> a;
    for (int64_t i = 0; i < T_steps; ++i) {
        StepOpts o;
        o.k_offset = k_offset; o.plant_feedback = 1;
        int sp, rc = comm_take_slot(h, o, sp);
        if (rc) return rc;
        fill_args<T>(h, a, d_state, (const char *)d_pools + (size_t)(i % n_pools) * pool_bytes, h->d_result, g, o);
        p.step = i;
        const hipError_t e = launch_rollout<T>(h, k, a, 1, s, &p);                                           // one epoch per step
        if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "sharded closed-loop launch failed: %s", hipGetErrorString(e));
        comm_submit(h, sp, o, d_results + (size_t)i * R, i + 1 < T_steps ? p.ring : nullptr, p.seq_theta, (long long)(i + 1));
    }
    int rc = rovmpc_comm_join(h, s);
    if (rc) return rc;
    hipLaunchKernelGGL(final_state_kernel, dim3(1), dim3(64), 0, s, d_state, d_exo, (const double *)d_results, (long long)T_steps, (int)R, 1);
    HIPCHK(h, hipGetLastError());
    return ROVMPC_OK;
}

extern "C" int rovmpc_closed_loop_pipelined_device(rovmpc_handle *h, const double *d_exo, int64_t T, double *d_state,
                                                   const void *d_pools, int32_t n_pools, int32_t feedback, double *d_results,
                                                   void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    h->cl_form = 0;
    if (T < 1 || n_pools < 1 || !d_exo || !d_state || !d_pools || !d_results)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_closed_loop_pipelined_device: bad argument");
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->comm) FAIL(h, ROVMPC_ERR_UNSUPPORTED, "pipelined closed loop is single-GPU: the sharded loop needs a host-issued collective per step");
    if (feedback && h->cfg.feature_map == ROVMPC_FEATURES_GEN3)
        FAIL(h, ROVMPC_ERR_UNSUPPORTED, "closed loop with model feedback carries (theta, gamma) only (see rovmpc_closed_loop_device)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return h->cfg.dtype == ROVMPC_F64
               ? closed_loop_pipelined_t<double>(h, d_exo, T, d_state, d_pools, n_pools, feedback, d_results, (hipStream_t)stream)
               : closed_loop_pipelined_t<float>(h, d_exo, T, d_state, d_pools, n_pools, feedback, d_results, (hipStream_t)stream);
}

extern "C" int rovmpc_closed_loop_device(rovmpc_handle *h, const double *d_exo, int64_t T, double *d_state, const void *d_pools,
                                         int32_t n_pools, int64_t k_offset, int32_t feedback, double *d_results, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    h->cl_form = 0;
    if (T < 1 || n_pools < 1 || !d_exo || !d_state || !d_pools || !d_results)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_closed_loop_device: bad argument");
    int rc = check_ready(h);
    if (rc) return rc;
    if (feedback && h->cfg.feature_map == ROVMPC_FEATURES_GEN3)
        FAIL(h, ROVMPC_ERR_UNSUPPORTED, "closed loop with model feedback carries (theta, gamma) only; the second-order map needs the rates "
                                        "(dtheta, dgamma) in state slots 14/15 -- supply measured rows (feedback = 0)");
    hipStream_t s = (hipStream_t)stream;
    const size_t R = rovmpc_result_len(h);
    const size_t pool_bytes = (size_t)h->cfg.K * h->cfg.N * 3 * h->esz;
    if (!h->comm) {
        // one GPU: the plant update of step i + 1 rides on the epilogue of step i (sweeping workgroup), so the
        // loop is back-to-back rollout kernels; only step 0 needs the stand-alone update
        h->cl_form = 1;
        hipLaunchKernelGGL(plant_update_kernel, dim3(1), dim3(64), 0, s, d_state, d_exo, (const double *)nullptr);
        HIPCHK(h, hipGetLastError());
        for (int64_t i = 0; i < T; ++i) {
            const void *U = (const char *)d_pools + (size_t)(i % n_pools) * pool_bytes;
            StepOpts o;
            o.plant_next = i + 1 < T ? d_exo + (size_t)(i + 1) * 16 : nullptr;
            o.plant_state = d_state; o.plant_feedback = feedback ? 1 : 0;
            if ((rc = enqueue_step(h, d_state, U, d_results + (size_t)i * R, s, o))) return rc;
        }
        return ROVMPC_OK;
    }
    // model feedback over the sharded step: the GPU-side hand-off (closed_loop_sharded_handoff_t) unless the model runs on the
    // interpreter (no step kernel), ROVMPC_CL_JOIN asks for the join-based form below, or the step kernel's grid is not
    // resident in one round: step g + 1's workgroups spin on their CU slots until step g's select has run, so a grid of
    // several rounds would leave the all-reduce and select of step g nowhere to run (every step a hand-off time-out)
    if (feedback && T > 1 && !getenv("ROVMPC_CL_JOIN") &&
        (h->model_kind == MODEL_BUILTIN || (h->model_kind == MODEL_JIT && h->jit_fn_step))) {
        HIPCHK(h, hipSetDevice(h->cfg.device));
        const Geo g = launch_geometry(h, 1);
        Launchable k;
        const int capacity = step_kernel_capacity(h, g, k);
        const bool one_round = capacity > 0 && g.nblocks <= capacity;
        if (getenv("ROVMPC_CL_VERBOSE"))
            fprintf(stderr, "[rovmpc] sharded closed loop: %d workgroups, %d resident at once -> %s\n", g.nblocks, capacity,
                    one_round ? "GPU-side hand-off" : "join per step");
        if (one_round) {
            h->cl_form = 4;
            return h->cfg.dtype == ROVMPC_F64 ? closed_loop_sharded_handoff_t<double>(h, k, d_exo, T, d_state, d_pools, n_pools, k_offset, d_results, s)
                                              : closed_loop_sharded_handoff_t<float>(h, k, d_exo, T, d_state, d_pools, n_pools, k_offset, d_results, s);
        }
    }
    h->cl_form = 3;
    for (int64_t i = 0; i < T; ++i) {
        const double *prev = (feedback && i > 0) ? d_results + (size_t)(i - 1) * R : nullptr;
        if (prev) {
            // the previous global record is produced on the side stream
            rc = rovmpc_comm_join(h, s);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(plant_update_kernel, dim3(1), dim3(64), 0, s, d_state, d_exo + (size_t)i * 16, prev);
        HIPCHK(h, hipGetLastError());
        const void *U = (const char *)d_pools + (size_t)(i % n_pools) * pool_bytes;
        rc = rovmpc_step_device_allreduce(h, d_state, U, k_offset, d_results + (size_t)i * R, s);
        if (rc) return rc;
    }
    if (h->comm) return rovmpc_comm_join(h, s);
    return ROVMPC_OK;
}
