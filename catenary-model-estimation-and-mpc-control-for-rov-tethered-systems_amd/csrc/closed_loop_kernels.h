// closed_loop_kernels.h -- plant update and final state of the closed-loop forms (closed_loop_host.hip only: they are not
// templates).
#pragma once
#include "rollout_kernels.h"

namespace rovmpc {

// State the closed loop with GPU-side hand-off leaves behind when the records, not the state buffer, carried it from step to
// step: the state step T - 1 started from (rows: [T][16]; records: [T][R]).
__global__ void __launch_bounds__(64)
final_state_kernel(double *state, const double *rows, const double *records, long long T, int R, int feedback) {
    const int t = threadIdx.x;
    if (t >= 16) return;
    const double *row = rows + (size_t)(T - 1) * 16;
    double v = row[t];
    if (feedback && T >= 2 && t >= 12) {
        const double *rec = records + (size_t)(T - 2) * R;
        v = t == 12 ? rec[7] : t == 13 ? rec[8] : t == 14 ? rec[5] : rec[6];
    }
    state[t] = v;
}

// Plant update of the closed-loop driver (one tiny workgroup): exogenous slots from the measured
// trajectory row, (theta, gamma) advanced to the first predicted node of the previous winner.
__global__ void __launch_bounds__(64)
plant_update_kernel(double *state, const double *exo_row, const double *prev_result) {
    const int t = threadIdx.x;
    if (prev_result) {          // feedback: keep the model's own (theta, gamma), take the rest from the row
        if (t < 12) state[t] = exo_row[t];
        if (t == 12) {
            const double th = state[12], ga = state[13];
            state[14] = th; state[15] = ga;
            state[12] = prev_result[7]; state[13] = prev_result[8];   // record: [J, k, u(3), th0, ga0, th1, ga1, ...]
        }
    } else if (t < 16) {
        state[t] = exo_row[t];
    }
}

}  // namespace rovmpc
