// track_kernels.h -- (theta, gamma) along marker recordings on gfx950 (rovmpc_track_markers, rovmpc_track_markers_device): the
// chain of per-frame fits whose start is the last accepted estimate, one 64-lane wave per recording.  The law is stated in
// include/rovmpc.h above rovmpc_track_markers.  Every attempt is fit_frame of fit_kernels.h, called as it stands.
#pragma once
#include "fit_kernels.h"

namespace rovmpc {

// A workgroup is four waves, a wave takes the recording 4 blockIdx.x + (wave index) and walks its frames t0 .. t1 - 1 in
// order; nothing is shared between waves: no LDS, no barrier.  fit_frame returns the same bits in all 64 lanes, so every
// decision here (accepted or not, which start is next, the track state) is taken on wave-equal values and made scalar by a
// readfirstlane.  The carry lives in registers along the launch.  It enters from `carry` at frame 0 and from the previous
// frame's row of `out` at t0 > 0 (the output angles of a frame ARE the carry after it: the accepted estimate, the held
// carry, or NaN = none), so a launch boundary changes no bit.  Lane 0 writes.
// Bounded by construction: (t1 - t0) (1 + n_starts) (max_iter + 1) model evaluations per wave.
struct TrackArgs {
    const double *P0, *P1, *Y;              // [B][T][3], [B][T][3], [B][T][M][3]
    double *carry;                          // [B][2] in (read at t0 = 0) and out, or null
    double *out;                            // [B][T][ROVMPC_TRACK_OUT]
    double *exo;                            // [B][T][16] or null: slots 12..15 of the frames that are not NONE
    double L, c_lo, c_hi, up;               // as FitArgs
    double tol, rms_max;
    double starts[ROVMPC_TRACK_MAX_STARTS][2];
    long long B, T, t0, t1;                 // this launch: frames t0 <= t < t1 of every recording
    int M, max_iter, n_starts;
};

RV_DEV bool track_finite2(double a, double b) { return fit_uniform((a - a) + (b - b) == 0.0); }

__global__ void __launch_bounds__(FIT_NT) track_markers_kernel(const TrackArgs a) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * FIT_FRAMES + (threadIdx.x >> 6);
    if (b >= a.B) return;                                                   // the whole wave
    const double nan = __builtin_nan("");
    double cth = nan, cga = nan;
    if (a.t0 > 0) {
        const double *prev = a.out + ROVMPC_TRACK_OUT * (b * a.T + a.t0 - 1);
        cth = prev[0]; cga = prev[1];
    } else if (a.carry) {
        cth = a.carry[2 * b]; cga = a.carry[2 * b + 1];
    }
    for (long long t = a.t0; t < a.t1; ++t) {
        const long long f = b * a.T + t;
        const FitFrame q = fit_load(a.P0, a.P1, a.Y, f, a.M, a.L, a.c_lo, a.c_hi, a.up, lane);
        const bool have = track_finite2(cth, cga);
        if (!have) { cth = nan; cga = nan; }                                 // (a half-finite carry is none)
        FitResult r = {};
        int steps = 0, k = have ? -1 : 0;
        bool accepted = false;
        for (;; ++k) {
            r = fit_frame(q, a.tol, a.max_iter, k < 0 ? cth : a.starts[k][0], k < 0 ? cga : a.starts[k][1]);
            steps += r.iters;
            accepted = fit_uniform(r.status == ROVMPC_FIT_CONVERGED && r.rms <= a.rms_max);
            if (fit_uniform(accepted || r.status == ROVMPC_FIT_TOO_FEW || r.status == ROVMPC_FIT_NONFINITE) || k + 1 >= a.n_starts) break;
        }
        const int state = accepted ? (k < 0 ? ROVMPC_TRACK_LOCKED : ROVMPC_TRACK_ACQUIRED) : (have ? ROVMPC_TRACK_HELD : ROVMPC_TRACK_NONE);
        const double th = accepted ? r.th : cth, ga = accepted ? r.ga : cga;          // (HELD: the carry; NONE: NaN)
        const double pth = have ? cth : th, pga = have ? cga : ga;
        if (lane == 0) {
            double *o = a.out + ROVMPC_TRACK_OUT * f;
            o[0] = th; o[1] = ga; o[2] = pth; o[3] = pga; o[4] = accepted ? r.rms : nan; o[5] = (double)steps;
            o[6] = (double)r.status; o[7] = (double)state; o[8] = (double)k;
            if (a.exo && state != ROVMPC_TRACK_NONE) {
                double *e = a.exo + 16 * f + 12;
                e[0] = th; e[1] = ga; e[2] = pth; e[3] = pga;
            }
        }
        if (accepted) { cth = r.th; cga = r.ga; }
    }
    if (a.carry && lane == 0) { a.carry[2 * b] = cth; a.carry[2 * b + 1] = cga; }
}

}  // namespace rovmpc
