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

// ---- pipelined closed loop: one step per launch, launches alternating between two streams -----------------------
template <typename T, int VT>
static hipError_t launch_step(const rovmpc_handle *h, const RolloutArgs<T> &a, const HandoffArgs &p, hipStream_t s, bool probe, int *capacity) {
    const size_t lds = rollout_lds_elems<T>(a.N, a.CK, MODEL_BUILTIN, VT) * sizeof(T);
    auto kern = (a.CK == 16 && a.ck_shift == 4) ? closed_loop_step_kernel16<T, MODEL_BUILTIN, VT> : closed_loop_step_kernel<T, MODEL_BUILTIN, VT>;   // (literal-CK instance: rollout_body, CKC)
    if constexpr (sizeof(T) == 8) { if (a.CK == 16 && a.ck_shift == 4 && a.N == 20 && !getenv("ROVMPC_NO_LITERAL_N")) kern = closed_loop_step_kernel16_n20<T, MODEL_BUILTIN, VT>; }
    if (probe) {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        int per_cu = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kern, a.NT, lds);
        if (e != hipSuccess) return e;
        *capacity = per_cu * h->n_cu;
        return hipSuccess;
    }
    hipLaunchKernelGGL(kern, dim3(a.nblocks), dim3(a.NT), lds, s, a, p);
    return hipGetLastError();
}

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
    const int vt = h->cfg.vt_mode;
    const size_t R = rovmpc_result_len(h);
    RolloutArgs<T> a;
    HandoffArgs p;
    int rcw = closed_loop_workspace(h, p, s);
    if (rcw) return rcw;
    p.T = T_steps; p.exo = d_exo;
    const size_t pool_bytes = (size_t)h->cfg.K * h->cfg.N * 3 * sizeof(T);
    int capacity = 0;
    if (h->model_kind == MODEL_BUILTIN) {
        h->plant_feedback = 0;
        fill_args<T>(h, a, d_state, d_pools, nullptr, g, 1);
        --*h->epoch_ctr;                                         // (the probe takes no epoch)
        hipError_t e = vt == 0 ? launch_step<T, 0>(h, a, p, s, true, &capacity) : vt == 1 ? launch_step<T, 1>(h, a, p, s, true, &capacity)
                                                                                      : launch_step<T, 2>(h, a, p, s, true, &capacity);
        if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "occupancy query failed: %s", hipGetErrorString(e));
    } else if (h->model_kind == MODEL_JIT) {
        if (!h->jit_fn_step) FAIL(h, ROVMPC_ERR_UNSUPPORTED, "the run-time specialised module has no pipelined entry");
        const size_t lds = rollout_lds_elems<T>(h->cfg.N, g.CK, MODEL_JIT, vt, jit_lds_planes(h->used_planes, vt, h->cfg.feature_map), h->jit_gi) * sizeof(T);
        if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)h->jit_fn_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        int per_cu = 0;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->jit_fn_step, g.NT, lds) != hipSuccess) per_cu = 0;
        capacity = per_cu * h->n_cu;
    } else {
        FAIL(h, ROVMPC_ERR_UNSUPPORTED, "pipelined closed loop: compiled-in and hiprtc-specialised models only (the interpreter runs launch per step)");
    }
    if (2 * g.nblocks > capacity)
        FAIL(h, ROVMPC_ERR_UNSUPPORTED, "pipelined closed loop needs two grids resident at once: 2 x %d workgroups exceed the device's capacity %d "
                                        "(use rovmpc_closed_loop_device)", g.nblocks, capacity);
    h->cl_form = 2;
    hipLaunchKernelGGL(plant_update_kernel, dim3(1), dim3(64), 0, s, d_state, d_exo, (const double *)nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->pipe_ev[2], s));
    HIPCHK(h, hipStreamWaitEvent(h->pipe_streams[1], h->pipe_ev[2], 0));
    for (int64_t i = 0; i < T_steps; ++i) {
        hipStream_t st = (i & 1) ? h->pipe_streams[1] : s;
        h->plant_feedback = feedback ? 1 : 0;
        fill_args<T>(h, a, d_state, (const char *)d_pools + (size_t)(i % n_pools) * pool_bytes, nullptr, g, 1);   // one epoch per step
        h->plant_feedback = 0;
        a.result = d_results + (size_t)i * R; a.k_offset = 0; a.slots = nullptr; a.rank = 0; a.world = 1;
        a.sweeper = 0;
        p.step = i;
        const HandoffArgs &pi = p;
        hipError_t e;
        if (h->model_kind == MODEL_JIT) {
            const size_t lds = rollout_lds_elems<T>(a.N, a.CK, MODEL_JIT, vt, jit_lds_planes(h->used_planes, vt, h->cfg.feature_map), h->jit_gi) * sizeof(T);
            if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)h->jit_fn_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            struct { RolloutArgs<T> a; HandoffArgs p; } both{a, pi};
            size_t asz = sizeof(both);
            void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &both, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
            e = hipModuleLaunchKernel(h->jit_fn_step, a.nblocks, 1, 1, a.NT, 1, 1, (unsigned)lds, st, nullptr, extra);
        } else {
            e = vt == 0 ? launch_step<T, 0>(h, a, pi, st, false, &capacity) : vt == 1 ? launch_step<T, 1>(h, a, pi, st, false, &capacity)
                                                                                      : launch_step<T, 2>(h, a, pi, st, false, &capacity);
        }
        if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "pipelined closed-loop launch failed: %s", hipGetErrorString(e));
    }
    HIPCHK(h, hipEventRecord(h->pipe_ev[1], h->pipe_streams[1]));
    HIPCHK(h, hipStreamWaitEvent(s, h->pipe_ev[1], 0));
    return ROVMPC_OK;
}

// Workgroups of the closed-loop step kernel (the instance launch_step / jit_fn_step would run, with its dynamic LDS) the
// device holds at once: resident workgroups per CU x CUs; 0 if the model has no step kernel or the query fails.  Sets the
// kernel's dynamic-LDS attribute on the way, as the launches need.
template <typename T>
static int step_kernel_capacity(rovmpc_handle *h, const Geo &g) {
    const int vt = h->cfg.vt_mode;
    int capacity = 0;
    if (h->model_kind == MODEL_BUILTIN) {
        RolloutArgs<T> a;
        const HandoffArgs p{};
        fill_args<T>(h, a, nullptr, nullptr, nullptr, g, 1);
        --*h->epoch_ctr;                                         // (the probe takes no epoch)
        hipError_t e = vt == 0 ? launch_step<T, 0>(h, a, p, nullptr, true, &capacity) : vt == 1 ? launch_step<T, 1>(h, a, p, nullptr, true, &capacity)
                                                                                              : launch_step<T, 2>(h, a, p, nullptr, true, &capacity);
        if (e != hipSuccess) capacity = 0;
    } else if (h->model_kind == MODEL_JIT && h->jit_fn_step) {
        const size_t lds = rollout_lds_elems<T>(h->cfg.N, g.CK, MODEL_JIT, vt, jit_lds_planes(h->used_planes, vt, h->cfg.feature_map), h->jit_gi) * sizeof(T);
        if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)h->jit_fn_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        int per_cu = 0;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->jit_fn_step, g.NT, lds) != hipSuccess) per_cu = 0;
        capacity = per_cu * h->n_cu;
    }
    return capacity;
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
static int closed_loop_sharded_handoff_t(rovmpc_handle *h, const double *d_exo, int64_t T_steps, double *d_state, const void *d_pools,
                                         int32_t n_pools, int64_t k_offset, double *d_results, hipStream_t s) {
    const Geo g = launch_geometry(h, 1);
    const int vt = h->cfg.vt_mode;
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
        const int sp = h->comm_flip;
        h->comm_flip = (h->comm_flip + 1) % rovmpc_handle::NSLOT;
        if (h->slot_used[sp]) {
            int rc = comm_wait_enqueued(h, sp);
            if (rc) return rc;
        }
        h->slot_used[sp] = true;
        const unsigned long long use = ++h->slot_uses[sp];
        h->arg_flag_consumed = h->d_flags + rovmpc_handle::NSLOT + sp; h->arg_consumed_need = use - 1;
        h->arg_flag_rolled = h->d_flags + sp; h->arg_rolled_seq = use;
        h->arg_slot_bad = h->d_flags + 2 * rovmpc_handle::NSLOT + sp;
        int inject = 0;
        if (h->inject_skip_rolled > 0) { --h->inject_skip_rolled; inject |= 1; }
        if (h->inject_skip_consumed > 0) { --h->inject_skip_consumed; inject |= 2; }
        h->arg_inject = inject;
        h->plant_feedback = 1;
        fill_args<T>(h, a, d_state, (const char *)d_pools + (size_t)(i % n_pools) * pool_bytes, nullptr, g, 1);   // one epoch per step
        h->plant_feedback = 0;
        h->arg_flag_consumed = nullptr; h->arg_flag_rolled = nullptr; h->arg_slot_bad = nullptr; h->arg_inject = 0;
        a.result = h->d_result; a.k_offset = k_offset; a.slots = h->d_slots[sp]; a.rank = h->comm_rank; a.world = h->comm_world;
        p.step = i;
        hipError_t e;
        int capacity = 0;     // (not probed here: the caller's step_kernel_capacity has set the LDS attribute)
        if (h->model_kind == MODEL_JIT) {
            const size_t lds = rollout_lds_elems<T>(a.N, a.CK, MODEL_JIT, vt, jit_lds_planes(h->used_planes, vt, h->cfg.feature_map), h->jit_gi) * sizeof(T);
            if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)h->jit_fn_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            struct { RolloutArgs<T> a; HandoffArgs p; } both{a, p};
            size_t asz = sizeof(both);
            void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &both, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
            e = hipModuleLaunchKernel(h->jit_fn_step, a.nblocks, 1, 1, a.NT, 1, 1, (unsigned)lds, s, nullptr, extra);
        } else {
            e = vt == 0 ? launch_step<T, 0>(h, a, p, s, false, &capacity) : vt == 1 ? launch_step<T, 1>(h, a, p, s, false, &capacity)
                                                                          : launch_step<T, 2>(h, a, p, s, false, &capacity);
        }
        if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "sharded closed-loop launch failed: %s", hipGetErrorString(e));
        {
            std::lock_guard<std::mutex> lk(h->comm_mu);
            h->comm_q.push_back({sp, d_results + (size_t)i * R, use, (int)(h->comm_rr++ % (unsigned long long)h->ncomm), inject,
                                 i + 1 < T_steps ? p.ring : nullptr, p.seq_theta, (long long)(i + 1)});
            ++h->comm_submitted[sp];
        }
        h->comm_cv.notify_all();
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
            h->plant_next = i + 1 < T ? d_exo + (size_t)(i + 1) * 16 : nullptr;
            h->plant_state = d_state; h->plant_feedback = feedback ? 1 : 0;
            rc = enqueue_step(h, d_state, U, nullptr, d_results + (size_t)i * R, 0, nullptr, 0, 1, s);
            h->plant_next = nullptr; h->plant_state = nullptr; h->plant_feedback = 0;
            if (rc) return rc;
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
        const int capacity = h->cfg.dtype == ROVMPC_F64 ? step_kernel_capacity<double>(h, g) : step_kernel_capacity<float>(h, g);
        const bool one_round = capacity > 0 && g.nblocks <= capacity;
        if (getenv("ROVMPC_CL_VERBOSE"))
            fprintf(stderr, "[rovmpc] sharded closed loop: %d workgroups, %d resident at once -> %s\n", g.nblocks, capacity,
                    one_round ? "GPU-side hand-off" : "join per step");
        if (one_round) {
            h->cl_form = 4;
            return h->cfg.dtype == ROVMPC_F64 ? closed_loop_sharded_handoff_t<double>(h, d_exo, T, d_state, d_pools, n_pools, k_offset, d_results, s)
                                              : closed_loop_sharded_handoff_t<float>(h, d_exo, T, d_state, d_pools, n_pools, k_offset, d_results, s);
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
