// horizon_kernels.h -- rovmpc_score_pairs: Q (theta row, gamma row) pairs rolled H steps on their own predictions from every
// start row of B recordings, the error per horizon step reduced on the device (fp64, gfx950).  The law is in include/rovmpc.h;
// one workgroup per (pair, recording) walks its tiles of windows, the lane is the window; no atomics, nothing between workgroups.
#pragma once
#include "score_kernels.h"

namespace rovmpc {

constexpr int HORIZON_NT = ROVMPC_HORIZON_TILE;  // lanes per workgroup = windows per tile
static_assert(HORIZON_NT == SCORE_NT, "the tile's tree is the scoring tree");
constexpr int HORIZON_SUMS = 5;                  // n_ok, ss_theta, ss_gamma, ss_hold_theta, ss_hold_gamma through the tree
constexpr int HORIZON_RED = HORIZON_SUMS + 2;    // and the two maxima beside them
static_assert(ROVMPC_MAX_STACK >= HORIZON_RED, "the reduction reuses the operand stack's LDS");
static_assert(ROVMPC_MAX_FEATURES <= 64, "the named slots are one 64-bit mask");

// the named slots in the order of rovmpc_horizon_params
enum { HZ_THETA = 0, HZ_GAMMA, HZ_THETA_PREV, HZ_GAMMA_PREV, HZ_COS_THETA, HZ_SIN_GAMMA, HZ_SLOTS };

struct HorizonArgs {
    ScoreArgs t, g;                              // the two fronts' programs (len in t; X, time, T, B, F in t)
    const int32_t *pairs;                        // [Q][2]
    const double *theta, *gamma;                 // [B][T]
    double *skill, *pred;                        // [Q][B][H][ROVMPC_HORIZON_COLS], [Q][B][W][H][2] or null
    long long W;                                 // windows of a recording with n = T
    int H, stride, integrator, prev_mode;
    int slot[HZ_SLOTS];
    double mean[HZ_SLOTS], scale[HZ_SLOTS];      // of the named slots
};

// LDS in doubles: the operand stack (the tile's reduction afterwards) and the stage row
inline size_t horizon_lds_bytes(int F) { return (size_t)(ROVMPC_MAX_STACK + F) * HORIZON_NT * sizeof(double); }

// windows of a recording with n counted rows: s_w = w stride while s_w + H <= n - 1
__host__ __device__ inline long long horizon_windows(long long n, int H, int stride) {
    return n - 1 - H >= 0 ? (n - 1 - H) / stride + 1 : 0;
}

// score_tree_sum on HORIZON_SUMS columns at once (the same additions in the same order per column), the two maxima of the
// counted windows beside them: v[c][lane], all lanes call, results in v[c][0]
RV_DEV void horizon_tree(double *v, int lane) {
#pragma clang fp contract(off)
    constexpr int NT = HORIZON_NT;
    for (int s = NT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (lane < s) {
#pragma unroll
            for (int c = 0; c < HORIZON_SUMS; ++c) v[c * NT + lane] = v[c * NT + lane] + v[c * NT + lane + s];
#pragma unroll
            for (int c = HORIZON_SUMS; c < HORIZON_RED; ++c) {
                const double m0 = v[c * NT + lane], m1 = v[c * NT + lane + s];
                v[c * NT + lane] = m1 > m0 ? m1 : m0;
            }
        }
    }
    __syncthreads();
}

RV_DEV double horizon_scaled(double y, double mean, double scale) {
#pragma clang fp contract(off)
    return (y - mean) / scale;
}

__global__ void __launch_bounds__(HORIZON_NT)
score_pairs_kernel(const HorizonArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    constexpr int NT = HORIZON_NT;
    const int lane = threadIdx.x;
    double *const lds = reinterpret_cast<double *>(smem_raw);
    double *const stack = lds + lane;                                   // [ROVMPC_MAX_STACK][lane]
    double *const red = lds;                                            // [HORIZON_RED][NT]: the same LDS between two steps
    double *const feat = lds + (size_t)ROVMPC_MAX_STACK * NT + lane;    // [F][lane]
    const long long B = a.t.B, T = a.t.T;
    const long long q = blockIdx.x / B, b = blockIdx.x % B;
    const long long n = a.t.len ? a.t.len[b] : T;
    const int F = a.t.F, H = a.H, stride = a.stride;
    const bool rk4 = a.integrator == ROVMPC_RK4, hold = a.prev_mode == ROVMPC_PREV_HOLD;
    const int rt = a.pairs[2 * q], rg = a.pairs[2 * q + 1];
    const int32_t *code_t = a.t.code + a.t.code_off[rt], *code_g = a.g.code + a.g.code_off[rg];
    const int n_t = a.t.code_off[rt + 1] - a.t.code_off[rt], n_g = a.g.code_off[rg + 1] - a.g.code_off[rg];
    const double *consts_t = a.t.consts + a.t.const_off[rt], *consts_g = a.g.consts + a.g.const_off[rg];
    const double *X = a.t.X + (size_t)b * T * F, *time = a.t.time + (size_t)b * T;
    const double *theta = a.theta + (size_t)b * T, *gamma = a.gamma + (size_t)b * T;
    double *skill = a.skill + ((size_t)q * B + b) * H * ROVMPC_HORIZON_COLS;
    double *pred = a.pred ? a.pred + ((size_t)q * B + b) * a.W * H * 2 : nullptr;
    const double nan = m_nan<double>();
    const long long Wb = horizon_windows(n, H, stride);
    unsigned long long named = 0;
    for (int k = 0; k < HZ_SLOTS; ++k) if (a.slot[k] >= 0) named |= 1ull << a.slot[k];
    const int s_th = a.slot[HZ_THETA], s_ga = a.slot[HZ_GAMMA], s_thp = a.slot[HZ_THETA_PREV], s_gap = a.slot[HZ_GAMMA_PREV],
              s_cos = a.slot[HZ_COS_THETA], s_sin = a.slot[HZ_SIN_GAMMA];

    for (long long w0 = 0; w0 < Wb; w0 += NT) {
        const bool active = w0 + lane < Wb;
        const long long w = active ? w0 + lane : Wb - 1;                // windows past W_b repeat the last one: uniform control flow
        const long long s = w * stride;
        double th = theta[s], ga = gamma[s], thm = theta[s > 0 ? s - 1 : 0], gam = gamma[s > 0 ? s - 1 : 0];
        const double th0 = th, ga0 = ga;
        bool ok = true;                                                 // both predictions finite at every step so far
        for (int j = 1; j <= H; ++j) {
            const long long i = s + j;
            const double dt = time[i] - time[i - 1];
            const double *x0 = X + (i - 1) * F, *x1 = X + i * F;
            // the delay slots' two ends: the previous node and node i - 1, scaled
            const double pa_t = s_thp >= 0 ? horizon_scaled(thm, a.mean[HZ_THETA_PREV], a.scale[HZ_THETA_PREV]) : 0.0;
            const double pb_t = s_thp >= 0 ? horizon_scaled(th, a.mean[HZ_THETA_PREV], a.scale[HZ_THETA_PREV]) : 0.0;
            const double pa_g = s_gap >= 0 ? horizon_scaled(gam, a.mean[HZ_GAMMA_PREV], a.scale[HZ_GAMMA_PREV]) : 0.0;
            const double pb_g = s_gap >= 0 ? horizon_scaled(ga, a.mean[HZ_GAMMA_PREV], a.scale[HZ_GAMMA_PREV]) : 0.0;
            double kt = 0.0, kg = 0.0, acc_t = 0.0, acc_g = 0.0;
            const int stages = rk4 ? 4 : 1;
#pragma unroll 1
            for (int st = 0; st < stages; ++st) {
                const int c2 = st == 0 ? 0 : (st == 3 ? 2 : 1);         // 2 c
                // the stage state: y, y + (dt / 2) k1, y + (dt / 2) k2, y + dt k3
                const double hs = st == 3 ? dt : dt / 2;
                const double yth = st == 0 ? th : th + hs * kt, yga = st == 0 ? ga : ga + hs * kg;
                if (st != 2)                                            // (k3's exogenous slots are k2's)
                    for (int f = 0; f < F; ++f) {
                        if ((named >> f) & 1) continue;
                        feat[(size_t)f * NT] = c2 == 0 ? x0[f] : (c2 == 2 ? x1[f] : (x0[f] + x1[f]) / 2);
                    }
                feat[(size_t)s_th * NT] = horizon_scaled(yth, a.mean[HZ_THETA], a.scale[HZ_THETA]);
                feat[(size_t)s_ga * NT] = horizon_scaled(yga, a.mean[HZ_GAMMA], a.scale[HZ_GAMMA]);
                if (s_cos >= 0) feat[(size_t)s_cos * NT] = horizon_scaled(m_cos(yth), a.mean[HZ_COS_THETA], a.scale[HZ_COS_THETA]);
                if (s_sin >= 0) feat[(size_t)s_sin * NT] = horizon_scaled(m_sin(yga), a.mean[HZ_SIN_GAMMA], a.scale[HZ_SIN_GAMMA]);
                if (s_thp >= 0) feat[(size_t)s_thp * NT] = (hold || c2 == 0) ? pa_t : (c2 == 2 ? pb_t : (pa_t + pb_t) / 2);
                if (s_gap >= 0) feat[(size_t)s_gap * NT] = (hold || c2 == 0) ? pa_g : (c2 == 2 ? pb_g : (pa_g + pb_g) / 2);
                kt = interp_eval<double>(code_t, n_t, consts_t, feat, NT, stack, NT);
                kg = interp_eval<double>(code_g, n_g, consts_g, feat, NT, stack, NT);
                // ((k1 + 2 k2) + 2 k3) + k4, left to right
                const double wt = (st == 1 || st == 2) ? 2.0 : 1.0;
                acc_t = st == 0 ? kt : acc_t + wt * kt;
                acc_g = st == 0 ? kg : acc_g + wt * kg;
            }
            const double th_n = th + (rk4 ? (dt / 6) * acc_t : replay_euler_increment(acc_t, dt));
            const double ga_n = ga + (rk4 ? (dt / 6) * acc_g : replay_euler_increment(acc_g, dt));
            thm = th; gam = ga; th = th_n; ga = ga_n;
            ok = ok && m_finite(th) && m_finite(ga);
            if (pred && active) {
                double *p = pred + ((size_t)w * H + (j - 1)) * 2;
                p[0] = th; p[1] = ga;
            }
            // the tile's terms of step j through the tree (the operand stack is free until the next stage)
            const double yt = theta[i], yg = gamma[i];
            const bool counted = active && ok && m_finite(yt) && m_finite(yg);
            const double et = th - yt, eg = ga - yg, ht = th0 - yt, hg = ga0 - yg;
            red[lane] = counted ? 1.0 : 0.0;
            red[NT + lane] = counted ? et * et : 0.0;
            red[2 * NT + lane] = counted ? eg * eg : 0.0;
            red[3 * NT + lane] = counted ? ht * ht : 0.0;
            red[4 * NT + lane] = counted ? hg * hg : 0.0;
            red[5 * NT + lane] = counted ? m_abs(et) : 0.0;
            red[6 * NT + lane] = counted ? m_abs(eg) : 0.0;
            horizon_tree(red, lane);
            // lane 0 keeps the running sums over the tiles in the workgroup's own output rows, in increasing tile order from +0
            if (lane == 0) {
                double *o = skill + (size_t)(j - 1) * ROVMPC_HORIZON_COLS;
                const bool first = w0 == 0;
                const double mt = red[5 * NT], mg = red[6 * NT];
                o[4] = (first ? 0.0 : o[4]) + red[0];
                o[5] = (first ? 0.0 : o[5]) + red[NT];
                o[6] = (first ? 0.0 : o[6]) + red[2 * NT];
                o[7] = (first ? 0.0 : o[7]) + red[3 * NT];
                o[8] = (first ? 0.0 : o[8]) + red[4 * NT];
                o[2] = (first || mt > o[2]) ? mt : o[2];
                o[3] = (first || mg > o[3]) ? mg : o[3];
            }                                                           // (no barrier: red[c][0] is lane 0's own stack column)
        }
    }
    // entries of pred that belong to no window of this recording
    if (pred)
        for (long long e = Wb * H * 2 + lane; e < a.W * H * 2; e += NT) pred[e] = nan;
    // the columns from the sums (lane 0 wrote them itself)
    if (lane == 0)
        for (int j = 0; j < H; ++j) {
            double *o = skill + (size_t)j * ROVMPC_HORIZON_COLS;
            const double cnt = Wb > 0 ? o[4] : 0.0;
            if (cnt > 0.0) {
                o[0] = m_sqrt(o[5] / cnt);
                o[1] = m_sqrt(o[6] / cnt);
            } else {
                o[0] = o[1] = o[2] = o[3] = o[5] = o[6] = o[7] = o[8] = nan;
                o[4] = 0.0;
            }
        }
}

}  // namespace rovmpc
