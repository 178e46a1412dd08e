// comm_kernels.h -- kernels of the native collective's streams (one unit only, rovmpc.hip: they are not templates).
#pragma once
#include "rollout_kernels.h"

namespace rovmpc {

// After the all-reduce(min): every rank holds every rank's record; pick the lexicographic
// (cost, global index) minimum and decode it.
__global__ void __launch_bounds__(64)
select_kernel(const long long *slots, int world, int R, double *result, unsigned long long *flag_consumed = nullptr,
              unsigned long long consumed_seq = 0, const unsigned long long *slot_bad = nullptr, int inject = 0,
              double *ring = nullptr, unsigned long long *seq_theta = nullptr, long long step_next = 0) {
    __shared__ int s_r;
    if (threadIdx.x == 0) {
        double Jd = __builtin_inf(); double kd = __builtin_inf(); int rb = 0;
        for (int r = 0; r < world; ++r) {
            const double oJ = ordered_val(slots[(size_t)r * R]);
            const double ok = ordered_val(slots[(size_t)r * R + 1]);
            if (oJ < Jd || (oJ == Jd && ok < kd) || r == 0) { Jd = oJ; kd = ok; rb = r; }
        }
        s_r = rb;
    }
    __syncthreads();
    const int rb = s_r;
    // a hand-off of this use timed out (the row is not this step's): the record says so with a NaN cost
    const bool bad = slot_bad && ld_agent(slot_bad) == consumed_seq;
    for (int i = threadIdx.x; i < R; i += blockDim.x) result[i] = (bad && i == 0) ? __builtin_nan("") : ordered_val(slots[(size_t)rb * R + i]);
    // Sharded closed loop with the state handed over on the GPU: the rollout of step `step_next` is already launched and its
    // theta waves wait for this -- (theta, gamma) of its start = first predicted node of the GLOBAL winner, its delay slots =
    // what this step started from (record: [J, k, u(3), th0, ga0, th1, ga1, ...]); then the sequence word.  After a hand-off
    // that timed out the row is another step's: hand over NaN, so that every later record says so (theta NaN -> costs +inf)
    // instead of continuing, finite and wrong, from a stale state.
    if (ring && threadIdx.x == 0) {
        double *r4 = ring + (int)(step_next & 3) * 4;
        const double q = __builtin_nan("");
        st_agent(&r4[0], bad ? q : ordered_val(slots[(size_t)rb * R + 7])); st_agent(&r4[1], bad ? q : ordered_val(slots[(size_t)rb * R + 8]));
        st_agent(&r4[2], bad ? q : ordered_val(slots[(size_t)rb * R + 5])); st_agent(&r4[3], bad ? q : ordered_val(slots[(size_t)rb * R + 6]));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        st_agent(seq_theta, (unsigned long long)step_next);
    }
    if (flag_consumed && !(inject & 2)) {    // every read of the slot buffer is done: it may be rewritten
        __syncthreads();
        if (threadIdx.x == 0) st_agent(flag_consumed, consumed_seq);
    }
}

// Collective stream, ahead of the all-reduce of one step: wait until the rollout kernel of that step (running on the
// caller's stream) has published its row.  One lane polling with agent-scope loads; on giving up it raises the handle's
// error word and marks the use bad, so the step's record carries a NaN cost and rovmpc_comm_sync returns an error.
__global__ void __launch_bounds__(64)
wait_rolled_kernel(const unsigned long long *flag_rolled, unsigned long long seq, unsigned *err, unsigned long long *slot_bad,
                   unsigned long long handoff_ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long give_up = wall_clock64() + handoff_ticks;
    for (;;) {
        if (ld_agent(flag_rolled) >= seq) return;
        if (wall_clock64() > give_up) break;
        __builtin_amdgcn_s_sleep(16);
    }
    raise_error(err, ERR_WAIT_ROLLED);
    st_agent(slot_bad, seq);
}

// ---- placement probe of the collective streams (rovmpc.hip::place_comm_streams) ------------------------------------------
// A kernel that waits on one hardware queue can hold back the COMPLETION of kernels on another queue of the same
// command-processor pipe (queues k and k + 4 share one; tools/ubench/queue_collision.hip: +24 us per kernel).  The probe
// reproduces that on purpose: one lane parks on the candidate stream until `raise` (last on the caller's stream) lets it go
// or 2 ms pass; meanwhile a few short grids run back to back on the caller's stream.
__global__ void __launch_bounds__(64)
probe_park_kernel(const unsigned long long *flag, unsigned long long want, unsigned long long ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long give_up = wall_clock64() + ticks;
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        if (wall_clock64() > give_up) break;
        __builtin_amdgcn_s_sleep(16);
    }
}
__global__ void __launch_bounds__(64)
probe_short_kernel(double *x) {
    double v = x[blockIdx.x * 64 + threadIdx.x];
#pragma unroll 1
    for (int i = 0; i < 256; ++i) v = __builtin_fma(v, 1.0000001, 1e-9);
    x[blockIdx.x * 64 + threadIdx.x] = v;
}
__global__ void probe_raise_kernel(unsigned long long *flag, unsigned long long v) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace rovmpc
