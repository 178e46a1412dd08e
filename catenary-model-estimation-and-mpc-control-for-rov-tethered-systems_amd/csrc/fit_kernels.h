// fit_kernels.h -- (theta, gamma) of the augmented catenary cable from its markers on gfx950 (rovmpc_fit_theta_gamma,
// rovmpc_fit_theta_gamma_device): Levenberg-Marquardt on the 2 x 2 normal equations, one 64-lane wave per frame.  The law is
// stated in include/rovmpc.h above rovmpc_fit_theta_gamma.  The model is the tether cost's, called as it stands: tether_node
// and tether_sample of tether_kernels.h.
#pragma once
#include "tether_kernels.h"

namespace rovmpc {

// A workgroup is four waves, a wave takes the frame 4 blockIdx.x + (wave index), and nothing is shared between waves: no LDS,
// no barrier.  Lane 16 v + m of the wave evaluates sample m of the model at theta (v = 0), theta + h (v = 1), theta - h
// (v = 2); group 3 repeats group 0 (idle work: no divergence).  The 16 lanes of a group run tether_node for their variant
// redundantly -- the time of one lane, no broadcast -- and keep its parameters in registers (constant indices only).  Then
// every lane fetches the three points of its m by __shfl, forms the marker's row of J and r, and a 16-lane xor butterfly
// (8, 4, 2, 1: a + b on both partners, so all 16 lanes end with the same bits) adds the six sums.  All four groups hold the
// same three points per m, hence the same sums: every decision below is taken on values that are equal in all 64 lanes, and
// is made scalar by a readfirstlane.  One wave-wide model evaluation per trial step: the trial's group 0 is the next
// iterate's residual, its groups 1 and 2 the next Jacobian.
constexpr int FIT_NT = 256;
constexpr int FIT_FRAMES = FIT_NT / 64;     // frames per workgroup

struct FitArgs {
    const double *P0, *P1, *Y, *guess;      // [B][3], [B][3], [B][M][3], [B][2] or null
    double *out;                            // [B][ROVMPC_FIT_OUT]
    double L, c_lo, c_hi, up;               // L, c_lo, c_hi rounded to the handle's dtype, as the tether cost holds them
    double tol;
    long long B;
    int M, max_iter;
};

struct FitSums { double a, b, c, g0, g1, F; };      // J^T J = [[a, b], [b, c]], J^T r = (g0, g1), F = sum w |r|^2

RV_DEV double fit_butterfly(double s) {
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    return s;
}

RV_DEV double fit_dot(V3<double> p, V3<double> q) { return ::fma(p.x, q.x, ::fma(p.y, q.y, p.z * q.z)); }

RV_DEV bool fit_uniform(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }

// The model at (th, ga) on the wave: the six sums, whether the point is usable (a catenary, finite, at all three thetas) and
// whether the rotated end point at th itself is vertical (l' = 0: no catenary for any bracket).
RV_DEV bool fit_eval(const TetherArgs &t, V3<double> rel, double th, double ga, int v, int m, int ms, V3<double> y, bool wm, FitSums &S,
                     bool &vertical) {
    const double h = ROVMPC_FIT_H;
    const double thv = th + (v == 1 ? h : (v == 2 ? -h : 0.0));
    double par[TETHER_PAR];
    tether_node(t, rel, thv, ga, par);
    const V3<double> x = tether_sample(t, par, ms);
    const double flag = par[TP_FLAG];
    const bool usable = __shfl(flag, 0) == 1.0 && __shfl(flag, 16) == 1.0 && __shfl(flag, 32) == 1.0;
    vertical = fit_uniform(__shfl(par[TP_BX], 0) == 0.0 && __shfl(par[TP_BY], 0) == 0.0);
    const V3<double> x0 = {__shfl(x.x, m), __shfl(x.y, m), __shfl(x.z, m)};
    const V3<double> xp = {__shfl(x.x, 16 + m), __shfl(x.y, 16 + m), __shfl(x.z, 16 + m)};
    const V3<double> xm = {__shfl(x.x, 32 + m), __shfl(x.y, 32 + m), __shfl(x.z, 32 + m)};
    const double ih = 0.5 / h;                                              // 2^19
    const V3<double> jt = {(xp.x - xm.x) * ih, (xp.y - xm.y) * ih, (xp.z - xm.z) * ih};
    const V3<double> jg = cross3(V3<double>{par[TP_KGX], par[TP_KGY], par[TP_KGZ]}, x0);
    const V3<double> r = {x0.x - y.x, x0.y - y.y, x0.z - y.z};
    S.a = fit_butterfly(wm ? fit_dot(jt, jt) : 0.0);
    S.b = fit_butterfly(wm ? fit_dot(jt, jg) : 0.0);
    S.c = fit_butterfly(wm ? fit_dot(jg, jg) : 0.0);
    S.g0 = fit_butterfly(wm ? fit_dot(jt, r) : 0.0);
    S.g1 = fit_butterfly(wm ? fit_dot(jg, r) : 0.0);
    S.F = fit_butterfly(wm ? fit_dot(r, r) : 0.0);
    return fit_uniform(usable);
}

__global__ void __launch_bounds__(FIT_NT) fit_theta_gamma_kernel(const FitArgs a) {
    const int lane = threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * FIT_FRAMES + (threadIdx.x >> 6);
    if (f >= a.B) return;                                                   // the whole wave
    const int v = lane >> 4, m = lane & 15, M = a.M;
    const int ms = m < M ? m : M - 1;                                       // lanes beyond the markers repeat the last sample, weight 0

    TetherArgs t = {};
    t.L = a.L; t.c_lo = a.c_lo; t.c_hi = a.c_hi; t.up = a.up; t.M = M;
    const double *A = a.P0 + 3 * f, *P = a.P1 + 3 * f, *Yf = a.Y + (3 * f) * M + 3 * ms;
    const double Ax = A[0], Ay = A[1], Az = A[2];
    const V3<double> rel = {P[0] - Ax, P[1] - Ay, P[2] - Az};
    const V3<double> y = {Yf[0] - Ax, Yf[1] - Ay, Yf[2] - Az};
    const bool wm = m < M && m_finite(y.x) && m_finite(y.y) && m_finite(y.z);
    const double nw = fit_butterfly(wm ? 1.0 : 0.0);
    const double ni = fit_butterfly(wm && m > 0 && m < M - 1 ? 1.0 : 0.0);
    double th = a.guess ? a.guess[2 * f] : 0.0, ga = a.guess ? a.guess[2 * f + 1] : 0.0;
    double *out = a.out + ROVMPC_FIT_OUT * f;

    // (A - A) + ... is 0, or NaN once a coordinate of A, P or the start is non-finite
    const double fin = ((Ax - Ax) + (Ay - Ay) + (Az - Az)) + ((rel.x - rel.x) + (rel.y - rel.y) + (rel.z - rel.z)) + ((th - th) + (ga - ga));
    if (fit_uniform(fin != fin || (rel.x == 0.0 && rel.y == 0.0 && rel.z == 0.0))) {
        if (lane == 0) {
            const double q = __builtin_nan("");
            out[0] = q; out[1] = q; out[2] = q; out[3] = q; out[4] = 0.0; out[5] = (double)ROVMPC_FIT_NONFINITE;
        }
        return;
    }

    FitSums S = {}, St;
    double tht = th, gat = ga, dth = 0.0, dga = 0.0, mu = ROVMPC_FIT_MU0, F0 = 0.0;
    int iters = 0, status = ROVMPC_FIT_MAX_ITER;
    for (bool first = true;; first = false) {
        bool vertical;
        const bool usable = fit_eval(t, rel, tht, gat, v, m, ms, y, wm, St, vertical);
        bool moved = false;
        if (first) {
            S = St; F0 = St.F; moved = true;
            if (fit_uniform(ni == 0.0)) { status = ROVMPC_FIT_TOO_FEW; break; }
            if (!usable) { status = vertical ? ROVMPC_FIT_DEGENERATE : ROVMPC_FIT_CHORD; break; }
        } else {
            ++iters;
            moved = usable && fit_uniform(St.F <= S.F + (ROVMPC_FIT_SLACK * a.L) * ::sqrt(nw * S.F));
            if (moved) { th = tht; ga = gat; S = St; mu = ::fmax(mu * 0.1, ROVMPC_FIT_MU_MIN); } else mu *= 10.0;
            if (fit_uniform(::fmax(::fabs(dth), ::fabs(dga)) <= a.tol)) { status = ROVMPC_FIT_CONVERGED; break; }
        }
        if (moved && fit_uniform(!(S.a * S.c - S.b * S.b > ROVMPC_FIT_DET_MIN * S.a * S.c))) { status = ROVMPC_FIT_DEGENERATE; break; }
        if (iters >= a.max_iter) break;
        const double ad = S.a * (1.0 + mu), cd = S.c * (1.0 + mu), id = 1.0 / (ad * cd - S.b * S.b);
        dth = (S.g1 * S.b - S.g0 * cd) * id;
        dga = (S.g0 * S.b - S.g1 * ad) * id;
        tht = th + dth; gat = ga + dga;
    }
    if (lane == 0) {
        out[0] = th; out[1] = ga; out[2] = ::sqrt(S.F / nw); out[3] = ::sqrt(F0 / nw); out[4] = (double)iters; out[5] = (double)status;
    }
}

}  // namespace rovmpc
