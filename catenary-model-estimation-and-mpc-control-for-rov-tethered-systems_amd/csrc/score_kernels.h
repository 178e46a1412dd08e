// score_kernels.h -- rovmpc_score_rows: R expressions replayed along B recordings and reduced to scores on the device
// (fp64, gfx950).  The law is in include/rovmpc.h; one workgroup per (row, recording), no atomics, nothing between workgroups.
#pragma once
#include "util_kernels.h"

namespace rovmpc {

constexpr int SCORE_NT = ROVMPC_SCORE_TILE;      // lanes per workgroup = time rows per pass

struct ScoreArgs {
    const int32_t *code, *code_off;              // [code_off[R]], [R + 1]
    const double *consts;                        // [const_off[R]]
    const int32_t *const_off;                    // [R + 1]
    const double *X, *time, *truth, *target, *y0;   // [B][T][F], [B][T], [B][T], [B][T] or null, [B] or null
    const long long *len;                        // [B] or null
    double *scores, *est, *pred;                 // [R][B][ROVMPC_SCORE_COLS], [R][B][T] or null (both)
    long long T, B;
    int F, integrator;
};

// LDS in doubles: operand stack, the tile's p / increments (or dt) / e, and for RK4 the midpoint features
inline size_t score_lds_bytes(int F, int integrator) {
    return (size_t)(ROVMPC_MAX_STACK + 3 + (integrator == ROVMPC_RK4 ? F : 0)) * SCORE_NT * sizeof(double);
}

// the law's tree over the lanes: v[j] += v[j + s] for s = SCORE_NT / 2, ..., 1 (all lanes call; result in v[0])
RV_DEV void score_tree_sum(double *v, int lane) {
#pragma clang fp contract(off)
    for (int s = SCORE_NT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (lane < s) v[lane] = v[lane] + v[lane + s];
    }
    __syncthreads();
}

// sklearn's r2_score with force_finite
RV_DEV double score_r2(double ss_res, double ss_tot, long long n) {
#pragma clang fp contract(off)
    if (n < 2) return m_nan<double>();
    if (ss_tot == 0.0) return ss_res == 0.0 ? 1.0 : (ss_res != ss_res ? ss_res : 0.0);
    return 1.0 - ss_res / ss_tot;
}

__global__ void __launch_bounds__(SCORE_NT)
score_rows_kernel(const ScoreArgs a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    constexpr int NT = SCORE_NT;
    const int lane = threadIdx.x;
    double *const lds = reinterpret_cast<double *>(smem_raw);
    double *const stack = lds + lane;                                   // [ROVMPC_MAX_STACK][lane]
    double *const sP = lds + (size_t)ROVMPC_MAX_STACK * NT;             // p of the tile
    double *const sI = sP + NT;                                         // increments (first order) or dt (second order)
    double *const sE = sI + NT;                                         // e of the tile
    double *const feat = sE + NT + lane;                                // [F][lane], RK4 only
    __shared__ double sCarry;                                           // p of the last row of the tile before
    const long long r = blockIdx.x / a.B, b = blockIdx.x % a.B;
    const long long T = a.T, n = a.len ? a.len[b] : T;
    const int F = a.F, integ = a.integrator;
    const int32_t *code = a.code + a.code_off[r];
    const int ncode = a.code_off[r + 1] - a.code_off[r];
    const double *consts = a.consts + a.const_off[r];
    const double *X = a.X + (size_t)b * T * F, *time = a.time + (size_t)b * T, *truth = a.truth + (size_t)b * T;
    const double *target = a.target ? a.target + (size_t)b * T : nullptr;
    double *est = a.est ? a.est + ((size_t)r * a.B + b) * T : nullptr;
    double *pred = a.pred ? a.pred + ((size_t)r * a.B + b) * T : nullptr;
    const double nan = m_nan<double>();
    const bool first_order = integ == ROVMPC_RK4 || integ == ROVMPC_EULER;

    // first pass: the means of truth and target, lane j over rows j, j + NT, ... and the tree
    double ybar, gbar = 0.0;
    {
#pragma clang fp contract(off)
        double sy = 0.0, sg = 0.0;
        for (long long i = lane; i < n; i += NT) { sy = sy + truth[i]; if (target) sg = sg + target[i]; }
        sP[lane] = sy; sI[lane] = sg;
        score_tree_sum(sP, lane);
        score_tree_sum(sI, lane);
        ybar = sP[0] / (double)n; gbar = sI[0] / (double)n;
        __syncthreads();
    }

    double ss_res = 0.0, ss_tot = 0.0, ss_resp = 0.0, ss_totg = 0.0, mx = 0.0;
    long long first_bad = n;                                            // first row with a non-finite e
    bool bad_p = false;
    double y = 0.0, w = 0.0, dd_prev = 0.0;                             // the chain's state (thread 0)
    for (long long t0 = 0; t0 < n; t0 += NT) {
        const long long i0 = t0 + lane, i = i0 < n ? i0 : n - 1;        // rows past n repeat the last one: uniform control flow
        const long long im = i > 0 ? i - 1 : 0;
        // phase A: p at the rows, k2 at the feature midpoints
        const double p = interp_eval<double>(code, ncode, consts, X + i * F, 1, stack, NT);
        sP[lane] = p;
        const double dt = time[i] - time[im];
        double k2 = 0.0;
        if (integ == ROVMPC_RK4) {
            const double *x0 = X + im * F, *x1 = X + i * F;
            for (int f = 0; f < F; ++f) feat[(size_t)f * NT] = (x0[f] + x1[f]) / 2;       // simulate_rk4_theta_gamma.py:62-63
            k2 = interp_eval<double>(code, ncode, consts, feat, NT, stack, NT);
        }
        __syncthreads();
        if (first_order) {
            const double k1 = lane > 0 ? sP[lane - 1] : sCarry;         // k4 of step i - 1 (unused at i = 0)
            sI[lane] = integ == ROVMPC_RK4 ? replay_rk4_increment(dt, k1, k2, p) : replay_euler_increment(k1, dt);
        } else {
            sI[lane] = dt;
        }
        __syncthreads();
        // phase B: the reference's sequential recurrence, one lane
        if (lane == 0) {
            const int cnt = (int)(n - t0 < NT ? n - t0 : NT);
            int j = 0;
            if (t0 == 0) { y = a.y0 ? a.y0[b] : truth[0]; w = 0.0; dd_prev = sP[0]; sE[0] = y; j = 1; }
            if (first_order) {
                for (; j < cnt; ++j) { y = y + sI[j]; sE[j] = y; }
            } else {
                for (; j < cnt; ++j) {
                    const double dd = sP[j];
                    replay_second_order_step(integ, dd_prev, dd, sI[j], y, w);
                    dd_prev = dd;
                    sE[j] = y;
                }
            }
            sCarry = sP[NT - 1];
        }
        __syncthreads();
        // phase C: partial sums per lane, tile after tile
        if (i0 < n) {
#pragma clang fp contract(off)
            const double e = sE[lane], yt = truth[i0];
            const double d = yt - e, c = yt - ybar, ad = m_abs(d);
            ss_res = ss_res + d * d;
            ss_tot = ss_tot + c * c;
            mx = (ad > mx || ad != ad) ? ad : mx;
            if (!m_finite(e) && i0 < first_bad) first_bad = i0;
            if (target) {
                const double g = target[i0], dp = g - p, cg = g - gbar;
                ss_resp = ss_resp + dp * dp;
                ss_totg = ss_totg + cg * cg;
                bad_p = bad_p || !m_finite(p);
            }
            if (est) est[i0] = e;
            if (pred) pred[i0] = p;
        }
    }
    for (long long i = n + lane; i < T; i += NT) {
        if (est) est[i] = nan;
        if (pred) pred[i] = nan;
    }

    // one fixed tree over the lanes (the operand stack's LDS is free now)
    __syncthreads();
    static_assert(ROVMPC_MAX_STACK >= 7, "the reduction reuses the operand stack's LDS");
    double *red = lds;                                                  // [7][NT]
    red[lane] = ss_res; red[NT + lane] = ss_tot; red[2 * NT + lane] = ss_resp; red[3 * NT + lane] = ss_totg;
    red[4 * NT + lane] = mx; red[5 * NT + lane] = (double)first_bad; red[6 * NT + lane] = bad_p ? 1.0 : 0.0;   // (rows < 2^53: exact)
    for (int k = 0; k < 4; ++k) score_tree_sum(red + k * NT, lane);
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (lane < s) {
            const double m0 = red[4 * NT + lane], m1 = red[4 * NT + lane + s];
            red[4 * NT + lane] = (m1 > m0 || m1 != m1) ? m1 : m0;
            const double f0 = red[5 * NT + lane], f1 = red[5 * NT + lane + s];
            red[5 * NT + lane] = f1 < f0 ? f1 : f0;
            const double b0 = red[6 * NT + lane], b1 = red[6 * NT + lane + s];
            red[6 * NT + lane] = b1 > b0 ? b1 : b0;
        }
        __syncthreads();
    }
    if (lane == 0) {
#pragma clang fp contract(off)
        const double nf = red[5 * NT];
        const bool e_ok = nf >= (double)n, p_ok = target && red[6 * NT] == 0.0;
        const double res = red[0], dn = (double)n;
        double *s = a.scores + ((size_t)r * a.B + b) * ROVMPC_SCORE_COLS;
        s[0] = e_ok ? score_r2(res, red[NT], n) : nan;
        s[1] = e_ok ? m_sqrt(res / dn) : nan;
        s[2] = e_ok ? red[4 * NT] : nan;
        s[3] = nf;
        s[4] = p_ok ? red[2 * NT] / dn : nan;
        s[5] = p_ok ? score_r2(red[2 * NT], red[3 * NT], n) : nan;
        s[6] = e_ok ? y : nan;
        s[7] = e_ok ? res : nan;
    }
}

}  // namespace rovmpc
