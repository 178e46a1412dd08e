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

// One frame as its wave holds it: the lane's role (variant v, sample m, ms the sample it evaluates), the frame relative to A,
// the lane's marker and weight, the counts of valid and of valid interior markers, and `fin`, which is 0, or NaN once a
// coordinate of A or P is non-finite ((A - A) + ...).
struct FitFrame {
    TetherArgs t;
    V3<double> rel, y;
    double nw, ni, fin;
    int v, m, ms;
    bool wm;
};

struct FitResult { double th, ga, rms, rms0; int iters, status; };

// Frame f of P0[.][3], P1[.][3], Y[.][M][3].
RV_DEV FitFrame fit_load(const double *P0, const double *P1, const double *Y, long long f, int M, double L, double c_lo, double c_hi,
                         double up, int lane) {
    FitFrame q;
    q.v = lane >> 4; q.m = lane & 15;
    q.ms = q.m < M ? q.m : M - 1;                                           // lanes beyond the markers repeat the last sample, weight 0
    q.t = TetherArgs{};
    q.t.L = L; q.t.c_lo = c_lo; q.t.c_hi = c_hi; q.t.up = up; q.t.M = M;
    const double *A = P0 + 3 * f, *P = P1 + 3 * f, *Yf = Y + (3 * f) * M + 3 * q.ms;
    const double Ax = A[0], Ay = A[1], Az = A[2];
    q.rel = {P[0] - Ax, P[1] - Ay, P[2] - Az};
    q.y = {Yf[0] - Ax, Yf[1] - Ay, Yf[2] - Az};
    q.wm = q.m < M && m_finite(q.y.x) && m_finite(q.y.y) && m_finite(q.y.z);
    q.nw = fit_butterfly(q.wm ? 1.0 : 0.0);
    q.ni = fit_butterfly(q.wm && q.m > 0 && q.m < M - 1 ? 1.0 : 0.0);
    q.fin = ((Ax - Ax) + (Ay - Ay) + (Az - Az)) + ((q.rel.x - q.rel.x) + (q.rel.y - q.rel.y) + (q.rel.z - q.rel.z));
    return q;
}

// The law of rovmpc_fit_theta_gamma for one frame from the start (th, ga), on the whole wave: every lane returns the same
// bits.  Both kernels that fit (fit_theta_gamma_kernel, track_markers_kernel of track_kernels.h) call this and nothing else.
RV_DEV FitResult fit_frame(const FitFrame &q, double tol, int max_iter, double th, double ga) {
    const double fin = q.fin + ((th - th) + (ga - ga));                     // NaN once the start is non-finite too
    if (fit_uniform(fin != fin || (q.rel.x == 0.0 && q.rel.y == 0.0 && q.rel.z == 0.0))) {
        const double n = __builtin_nan("");
        return {n, n, n, n, 0, ROVMPC_FIT_NONFINITE};
    }
    const double nw = q.nw;
    FitSums S = {}, St;
    double tht = th, gat = ga, dth = 0.0, dga = 0.0, mu = ROVMPC_FIT_MU0, F0 = 0.0;
    int iters = 0, status = ROVMPC_FIT_MAX_ITER;
    for (bool first = true;; first = false) {
        bool vertical;
        const bool usable = fit_eval(q.t, q.rel, tht, gat, q.v, q.m, q.ms, q.y, q.wm, St, vertical);
        bool moved = false;
        if (first) {
            S = St; F0 = St.F; moved = true;
            if (fit_uniform(q.ni == 0.0)) { status = ROVMPC_FIT_TOO_FEW; break; }
            if (!usable) { status = vertical ? ROVMPC_FIT_DEGENERATE : ROVMPC_FIT_CHORD; break; }
        } else {
            ++iters;
            moved = usable && fit_uniform(St.F <= S.F + (ROVMPC_FIT_SLACK * q.t.L) * ::sqrt(nw * S.F));
            if (moved) { th = tht; ga = gat; S = St; mu = ::fmax(mu * 0.1, ROVMPC_FIT_MU_MIN); } else mu *= 10.0;
            if (fit_uniform(::fmax(::fabs(dth), ::fabs(dga)) <= tol)) { status = ROVMPC_FIT_CONVERGED; break; }
        }
        if (moved && fit_uniform(!(S.a * S.c - S.b * S.b > ROVMPC_FIT_DET_MIN * S.a * S.c))) { status = ROVMPC_FIT_DEGENERATE; break; }
        if (iters >= max_iter) break;
        const double ad = S.a * (1.0 + mu), cd = S.c * (1.0 + mu), id = 1.0 / (ad * cd - S.b * S.b);
        dth = (S.g1 * S.b - S.g0 * cd) * id;
        dga = (S.g0 * S.b - S.g1 * ad) * id;
        tht = th + dth; gat = ga + dga;
    }
    return {th, ga, ::sqrt(S.F / nw), ::sqrt(F0 / nw), iters, status};
}

__global__ void __launch_bounds__(FIT_NT) fit_theta_gamma_kernel(const FitArgs a) {
    const int lane = threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * FIT_FRAMES + (threadIdx.x >> 6);
    if (f >= a.B) return;                                                   // the whole wave
    const FitFrame q = fit_load(a.P0, a.P1, a.Y, f, a.M, a.L, a.c_lo, a.c_hi, a.up, lane);
    const FitResult r = fit_frame(q, a.tol, a.max_iter, a.guess ? a.guess[2 * f] : 0.0, a.guess ? a.guess[2 * f + 1] : 0.0);
    if (lane == 0) {
        double *out = a.out + ROVMPC_FIT_OUT * f;
        out[0] = r.th; out[1] = r.ga; out[2] = r.rms; out[3] = r.rms0; out[4] = (double)r.iters; out[5] = (double)r.status;
    }
}

}  // namespace rovmpc
