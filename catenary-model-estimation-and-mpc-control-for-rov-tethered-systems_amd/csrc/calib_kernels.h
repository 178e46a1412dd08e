// calib_kernels.h -- the cable length from marker recordings on gfx950 (rovmpc_calibrate_cable, rovmpc_calibrate_cable_device)
// and the forward model with markers placed by arc length (rovmpc_cable_markers).  The law is stated in include/rovmpc.h
// above rovmpc_calibrate_cable.  The model is the fit's: fit_load, tether_node, fit_butterfly, fit_dot are called as they
// stand, and with arc = NULL the sample is tether_sample itself.
#pragma once
#include "fit_kernels.h"

namespace rovmpc {

// asinh for the marker placement: sign(x) log1p(|x| + x^2 / (1 + sqrt(1 + x^2))).  The argument of log1p is formed without
// cancellation, so the relative error is a few ulp from |x| = 2^-60 (log1p(a) = a) up to the largest argument the placement
// forms, sinh(c_hi L / 2 + atanh(.)) (x^2 overflows only beyond 1e154).
RV_DEV double m_asinh(double x) {
    const double a = ::fabs(x), a2 = a * a;
    const double r = ::log1p(a + a2 / (1.0 + ::sqrt(1.0 + a2)));
    return x < 0.0 ? -r : r;
}

// Sample m of the node `par` with the markers placed by arc length: `s` is the marker's fraction of the cable's length.
// tether_sample's formula at the chord parameter the law gives; the end markers exactly at t = 0 and t = 1.
RV_DEV V3<double> calib_sample_arc(const TetherArgs &a, const double *par, int m, double s) {
    const double flag = par[TP_FLAG];
    if (flag != flag) return {flag, flag, flag};
    if (flag == 0.0) return {s * par[TP_RX], s * par[TP_RY], s * par[TP_RZ]};
    const double u = par[TP_U], w = u - par[TP_ATH];
    double t = (w + m_asinh(s * ((2.0 * a.L) / par[TP_2IC]) - m_sinh(w))) / (2.0 * u);
    t = m == 0 ? 0.0 : (m == a.M - 1 ? 1.0 : t);
    const double z = par[TP_2IC] * (m_sinh(u * t) * m_sinh(::fma(u, t - 1.0, par[TP_ATH])));
    V3<double> q = {t * par[TP_BX], t * par[TP_BY], a.up * z};
    q = rodrigues_unit(q, V3<double>{par[TP_KTX], par[TP_KTY], 0.0}, -par[TP_ST], par[TP_CT]);
    return rodrigues_unit(q, V3<double>{par[TP_KGX], par[TP_KGY], par[TP_KGZ]}, par[TP_SG], par[TP_CG]);
}

// ---- the forward model: one thread per (cable, marker) ------------------------------------------------------------------

struct MarkersArgs {
    const double *P0, *P1, *theta, *gamma, *Lb;     // [B][3], [B][3], [B], [B], [B] or null (L below)
    double *out;                                    // [B][M][3]
    double arc[ROVMPC_FIT_MAX_MARKERS];
    double L, c_lo, c_hi, up;
    long long B;
    int M, has_arc;
};

__global__ void __launch_bounds__(256) cable_markers_kernel(const MarkersArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.B * a.M) return;
    const long long b = i / a.M;
    const int m = (int)(i - b * a.M);
    TetherArgs t = TetherArgs{};
    t.L = a.Lb ? a.Lb[b] : a.L; t.c_lo = a.c_lo; t.c_hi = a.c_hi; t.up = a.up; t.M = a.M;
    const double *A = a.P0 + 3 * b, *P = a.P1 + 3 * b;
    const double Ax = A[0], Ay = A[1], Az = A[2];
    double par[TETHER_PAR];
    tether_node(t, V3<double>{P[0] - Ax, P[1] - Ay, P[2] - Az}, a.theta[b], a.gamma[b], par);
    const V3<double> x = a.has_arc ? calib_sample_arc(t, par, m, a.arc[m]) : tether_sample(t, par, m);
    double *o = a.out + 3 * i;
    o[0] = x.x + Ax; o[1] = x.y + Ay; o[2] = x.z + Az;
}

// ---- the calibration ------------------------------------------------------------------------------------------------------
// A trial step is a pair of launches.  calib_frames_kernel: one wave per frame, four frames per workgroup, evaluates the
// frame's trial point and leaves its ten sums and its usable flag in the frame's trial record.  calib_reduce_kernel: one
// workgroup per group adds the records in the law's order, decides, promotes trial records to iterate records, forms S, R,
// dL and writes every frame's next trial point, lanes across frames.  Launch 0 of the pair evaluates the start and
// classifies the frames.  A group's done word makes both kernels return at once for it.  Nothing waits on another workgroup.
//
// Records: structure of arrays in the handle's working buffer, field-major ([field][F] doubles), so that the reduce
// kernel's lanes read consecutive frames.
enum { CF_CLASS = 0,                        // -1 active, else the rovmpc_fit_status the frame was left out with
       CF_TH, CF_GA, CF_THT, CF_GAT,        // iterate, trial point
       CF_NW, CF_F0, CF_STEP,               // valid markers, F at the start, max(|dtheta|, |dgamma|) of the trial step
       CF_IT,                               // iterate sums: a b c g0 g1 F p0 p1 d gL
       CF_TR = CF_IT + 10,                  // trial sums, the same ten
       CF_USABLE = CF_TR + 10,
       CF_FIELDS };
enum { CG_L = 0, CG_LT, CG_DL, CG_MU, CG_ITERS, CG_F, CG_F0, CG_NW, CG_NACT, CG_FIELDS = 16 };

constexpr int CALIB_RNT = 8 * ROVMPC_SCORE_TILE;    // threads of the reduce kernel: one per frame of eight tiles

struct CalibArgs {
    const double *P0, *P1, *Y, *guess;      // [F][3], [F][3], [F][M][3], [F][2] or null
    const int *group_off;                   // [G + 1]
    double *rec, *grp;                      // [CF_FIELDS][F], [G][CG_FIELDS]
    int *done;                              // [G]
    double *out_group, *out_frame;          // [G][ROVMPC_CALIB_GROUP_OUT], [F][ROVMPC_CALIB_FRAME_OUT]
    double arc[ROVMPC_FIT_MAX_MARKERS];
    double L0, L_lo, L_hi, c_lo, c_hi, up, tol, tol_L;
    long long F;
    int G, M, max_iter, free_length, has_arc, launch;   // launch: 0 evaluates the start, k > 0 trial step k
};

struct CalibSums { double v[10]; };         // a b c g0 g1 F p0 p1 d gL

// the group of frame f: the g with group_off[g] <= f < group_off[g + 1]
RV_DEV int calib_group_of(const int *off, int G, long long f) {
    int lo = 0, hi = G;                     // off[lo] <= f < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)off[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

// the fit's test of a frame's 2 x 2 block, as its kernel rounds it
RV_DEV bool calib_det_ok(double sa, double sb, double sc) { return ::fma(sa, sc, -(sb * sb)) > ROVMPC_FIT_DET_MIN * sa * sc; }

// The model at (th, ga, L) on the wave, as fit_eval forms it (same lane map, same expressions): groups 0, 1, 2 of 16 lanes
// evaluate theta, theta + h, theta - h; with a free length group 3, idle in the fit, evaluates L + h, and a second evaluation
// (all lanes alike) L - h.  Returns usable.
RV_DEV bool calib_eval(const CalibArgs &a, const FitFrame &q, double sm, double th, double ga, double L, CalibSums &S, bool &vertical) {
    const double h = ROVMPC_FIT_H;
    const int v = q.v, m = q.m;
    const double thv = th + (v == 1 ? h : (v == 2 ? -h : 0.0));
    TetherArgs t = q.t;
    t.L = a.free_length && v == 3 ? L + h : L;
    double par[TETHER_PAR];
    tether_node(t, q.rel, thv, ga, par);
    const V3<double> x = a.has_arc ? calib_sample_arc(t, par, q.ms, sm) : tether_sample(t, par, q.ms);
    const double flag = par[TP_FLAG];
    bool usable = __shfl(flag, 0) == 1.0 && __shfl(flag, 16) == 1.0 && __shfl(flag, 32) == 1.0;
    vertical = fit_uniform(__shfl(par[TP_BX], 0) == 0.0 && __shfl(par[TP_BY], 0) == 0.0);
    const V3<double> x0 = {__shfl(x.x, m), __shfl(x.y, m), __shfl(x.z, m)};
    const V3<double> xp = {__shfl(x.x, 16 + m), __shfl(x.y, 16 + m), __shfl(x.z, 16 + m)};
    const V3<double> xm = {__shfl(x.x, 32 + m), __shfl(x.y, 32 + m), __shfl(x.z, 32 + m)};
    const double ih = 0.5 / h;                                              // 2^19
    const V3<double> jt = {(xp.x - xm.x) * ih, (xp.y - xm.y) * ih, (xp.z - xm.z) * ih};
    const V3<double> jg = cross3(V3<double>{par[TP_KGX], par[TP_KGY], par[TP_KGZ]}, x0);
    const V3<double> y = q.y;
    const V3<double> r = {x0.x - y.x, x0.y - y.y, x0.z - y.z};
    const bool wm = q.wm;
    S.v[0] = fit_butterfly(wm ? fit_dot(jt, jt) : 0.0);
    S.v[1] = fit_butterfly(wm ? fit_dot(jt, jg) : 0.0);
    S.v[2] = fit_butterfly(wm ? fit_dot(jg, jg) : 0.0);
    S.v[3] = fit_butterfly(wm ? fit_dot(jt, r) : 0.0);
    S.v[4] = fit_butterfly(wm ? fit_dot(jg, r) : 0.0);
    S.v[5] = fit_butterfly(wm ? fit_dot(r, r) : 0.0);
    S.v[6] = S.v[7] = S.v[8] = S.v[9] = 0.0;
    if (a.free_length) {                                                    // (uniform)
        const V3<double> xlp = {__shfl(x.x, 48 + m), __shfl(x.y, 48 + m), __shfl(x.z, 48 + m)};
        usable = usable && __shfl(flag, 48) == 1.0;
        t.L = L - h;
        double parm[TETHER_PAR];
        tether_node(t, q.rel, th, ga, parm);
        const V3<double> xlm = a.has_arc ? calib_sample_arc(t, parm, q.ms, sm) : tether_sample(t, parm, q.ms);
        usable = usable && parm[TP_FLAG] == 1.0;
        const V3<double> jl = {(xlp.x - xlm.x) * ih, (xlp.y - xlm.y) * ih, (xlp.z - xlm.z) * ih};
        S.v[6] = fit_butterfly(wm ? fit_dot(jt, jl) : 0.0);
        S.v[7] = fit_butterfly(wm ? fit_dot(jg, jl) : 0.0);
        S.v[8] = fit_butterfly(wm ? fit_dot(jl, jl) : 0.0);
        S.v[9] = fit_butterfly(wm ? fit_dot(jl, r) : 0.0);
    }
    return fit_uniform(usable);
}

__global__ void __launch_bounds__(FIT_NT) calib_frames_kernel(const CalibArgs a) {
    const int lane = threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * FIT_FRAMES + (threadIdx.x >> 6);
    if (f >= a.F) return;                                                   // the whole wave
    const int g = calib_group_of(a.group_off, a.G, f);
    const long long F = a.F;
    double *rec = a.rec + f;
    if (a.launch > 0 && (a.done[g] || rec[CF_CLASS * F] != -1.0)) return;
    const double L = a.launch ? a.grp[(size_t)g * CG_FIELDS + CG_LT] : a.L0;
    const FitFrame q = fit_load(a.P0, a.P1, a.Y, f, a.M, L, a.c_lo, a.c_hi, a.up, lane);
    const double sm = a.arc[q.ms];
    double th, ga;
    if (a.launch) { th = rec[CF_THT * F]; ga = rec[CF_GAT * F]; }
    else { th = a.guess ? a.guess[2 * f] : 0.0; ga = a.guess ? a.guess[2 * f + 1] : 0.0; }
    if (a.launch == 0) {
        const double fin = q.fin + ((th - th) + (ga - ga));                 // the fit's test, in its order
        if (fit_uniform(fin != fin || (q.rel.x == 0.0 && q.rel.y == 0.0 && q.rel.z == 0.0))) {
            if (lane == 0) {
                const double n = __builtin_nan("");
                double *o = a.out_frame + ROVMPC_CALIB_FRAME_OUT * f;
                o[0] = n; o[1] = n; o[2] = n; o[3] = n; o[4] = (double)ROVMPC_FIT_NONFINITE;
                rec[CF_CLASS * F] = (double)ROVMPC_FIT_NONFINITE;
            }
            return;
        }
    }
    CalibSums S;
    bool vertical;
    const bool usable = calib_eval(a, q, sm, th, ga, L, S, vertical);
    if (a.launch == 0) {
        int cls = -1;
        if (fit_uniform(q.ni == 0.0)) cls = ROVMPC_FIT_TOO_FEW;
        else if (!usable) cls = vertical ? ROVMPC_FIT_DEGENERATE : ROVMPC_FIT_CHORD;
        else if (fit_uniform(!calib_det_ok(S.v[0], S.v[1], S.v[2]))) cls = ROVMPC_FIT_DEGENERATE;
        if (lane == 0) {
            rec[CF_CLASS * F] = (double)cls;
            rec[CF_NW * F] = q.nw;
            rec[CF_F0 * F] = S.v[5];
            rec[CF_STEP * F] = 0.0;
            if (cls != -1) {
                const double rms = ::sqrt(S.v[5] / q.nw);
                double *o = a.out_frame + ROVMPC_CALIB_FRAME_OUT * f;
                o[0] = th; o[1] = ga; o[2] = rms; o[3] = rms; o[4] = (double)cls;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 10; ++i) rec[(CF_TR + i) * F] = S.v[i];
        rec[CF_USABLE * F] = usable ? 1.0 : 0.0;
    }
}

// Sums over the group's frames in the law's order: tiles of ROVMPC_SCORE_TILE consecutive frames, inside a tile the tree of
// rovmpc_score_rows, the tile sums added in tile order from +0.  NQ quantities at once; `term(f, x)` fills frame f's terms
// (an inactive frame's are 0).  The workgroup takes CALIB_TILES tiles at a time, two waves per tile: the tree's first level
// v[j] += v[j + 64] goes through LDS, the levels 32 .. 1 stay inside the tile's first wave (lane j takes lane j + s's value:
// the same additions), and every thread then adds the tile sums in tile order: the same bits in all threads.
constexpr int CALIB_TILES = CALIB_RNT / ROVMPC_SCORE_TILE;
constexpr int CALIB_NQ = 7;                                                 // the most quantities summed at once
constexpr int CALIB_LDS = CALIB_NQ * CALIB_TILES * (ROVMPC_SCORE_TILE / 2 + 1);   // doubles: the upper halves, then the tile sums

template <int NQ, typename Term>
RV_DEV void calib_group_sums(double *sm, long long f0, long long f1, int tid, Term term, double (&tot)[NQ]) {
    static_assert(NQ <= CALIB_NQ, "LDS of the reduce kernel");
    constexpr int HALF = ROVMPC_SCORE_TILE / 2;
    double *ts = sm + CALIB_NQ * CALIB_TILES * HALF;                        // [NQ][CALIB_TILES]
    const int tl = tid / ROVMPC_SCORE_TILE, j = tid % ROVMPC_SCORE_TILE;
    double acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.0;
    for (long long t0 = f0; t0 < f1; t0 += CALIB_RNT) {
        double x[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) x[i] = 0.0;
        if (t0 + tid < f1) term(t0 + tid, x);
        if (j >= HALF) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) sm[(i * CALIB_TILES + tl) * HALF + (j - HALF)] = x[i];
        }
        __syncthreads();
        if (j < HALF) {                                                     // (a whole wave)
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                double v = x[i] + sm[(i * CALIB_TILES + tl) * HALF + j];
                for (int s = HALF / 2; s >= 1; s >>= 1) v += __shfl_down(v, s);
                if (j == 0) ts[i * CALIB_TILES + tl] = v;
            }
        }
        __syncthreads();
        for (int k = 0; k < CALIB_TILES && t0 + (long long)k * ROVMPC_SCORE_TILE < f1; ++k) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) acc[i] += ts[i * CALIB_TILES + k];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) tot[i] = acc[i];
}

// The fit's Cramer expressions for -A'^-1 g at damping mu, with the roundings its kernel makes written out (every a b - c d
// below is one fma around the rounded second product; a step is the rounded product n / d, the fit's trial point the single
// fma(n, 1 / d, theta)): n0, n1 the numerators, id = 1 / d.
struct CalibStep { double n0, n1, id; };
RV_DEV CalibStep calib_solve(double sa, double sb, double sc, double g0, double g1, double mu) {
    const double ad = sa * (1.0 + mu), cd = sc * (1.0 + mu);
    return {::fma(sb, g1, -(g0 * cd)), ::fma(sb, g0, -(g1 * ad)), 1.0 / ::fma(ad, cd, -(sb * sb))};
}

__global__ void __launch_bounds__(CALIB_RNT) calib_reduce_kernel(const CalibArgs a) {
    __shared__ double sm[CALIB_LDS];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (a.launch > 0 && a.done[g]) return;                                  // the whole workgroup
    const long long F = a.F, f0 = a.group_off[g], f1 = a.group_off[g + 1];
    double *rec = a.rec, *grp = a.grp + (size_t)g * CG_FIELDS;
    const bool free_len = a.free_length != 0;

    // (1) the trial as a whole: sum F', frames not usable, the largest angle step; at launch 0 the counts as well
    double t1[6];
    calib_group_sums<6>(sm, f0, f1, tid, [&](long long f, double *x) {
        if (rec[CF_CLASS * F + f] != -1.0) return;
        x[0] = rec[(CF_TR + 5) * F + f];
        x[1] = rec[CF_USABLE * F + f] == 1.0 ? 0.0 : 1.0;
        x[2] = rec[CF_NW * F + f];
        x[3] = 1.0;
        x[4] = rec[CF_STEP * F + f] <= a.tol ? 0.0 : 1.0;                   // (a NaN step counts as large)
    }, t1);
    const double Ft = t1[0], Nw = t1[2], nact = t1[3];
    double L = a.launch ? grp[CG_L] : a.L0, mu = a.launch ? grp[CG_MU] : ROVMPC_FIT_MU0, Fg = a.launch ? grp[CG_F] : Ft;
    const double Lt = a.launch ? grp[CG_LT] : a.L0, dL = a.launch ? grp[CG_DL] : 0.0;
    const double F0 = a.launch ? grp[CG_F0] : Ft;
    int iters = a.launch, status = -1;
    bool moved;
    if (a.launch == 0) {
        moved = true;
        if (nact == 0.0) status = ROVMPC_CALIB_NO_FRAMES;
    } else {
        moved = t1[1] == 0.0 && (!free_len || (Lt > a.L_lo && Lt < a.L_hi)) && Ft <= ::fma(ROVMPC_FIT_SLACK * L, ::sqrt(Nw * Fg), Fg);
        if (moved) { L = Lt; Fg = Ft; mu = ::fmax(mu * 0.1, ROVMPC_FIT_MU_MIN); } else mu *= 10.0;
        if (t1[4] == 0.0 && ::fabs(dL) <= a.tol_L) status = ROVMPC_FIT_CONVERGED;
    }
    // promote: the trial records become the iterate's
    if (moved && status != ROVMPC_CALIB_NO_FRAMES)
        for (long long f = f0 + tid; f < f1; f += CALIB_RNT) {
            if (rec[CF_CLASS * F + f] != -1.0) continue;
            if (a.launch) { rec[CF_TH * F + f] = rec[CF_THT * F + f]; rec[CF_GA * F + f] = rec[CF_GAT * F + f]; }
            else { rec[CF_TH * F + f] = a.guess ? a.guess[2 * f] : 0.0; rec[CF_GA * F + f] = a.guess ? a.guess[2 * f + 1] : 0.0; }
#pragma unroll
            for (int i = 0; i < 10; ++i) rec[(CF_IT + i) * F + f] = rec[(CF_TR + i) * F + f];
        }
    __syncthreads();

    // (2) the Schur sums on the iterate at mu, and at 0 for sigma_L; frames whose 2 x 2 block is degenerate
    double t2[7];
    calib_group_sums<7>(sm, f0, f1, tid, [&](long long f, double *x) {
        if (rec[CF_CLASS * F + f] != -1.0) return;
        const double sa = rec[(CF_IT + 0) * F + f], sb = rec[(CF_IT + 1) * F + f], sc = rec[(CF_IT + 2) * F + f];
        const double g0 = rec[(CF_IT + 3) * F + f], g1 = rec[(CF_IT + 4) * F + f];
        const double p0 = rec[(CF_IT + 6) * F + f], p1 = rec[(CF_IT + 7) * F + f];
        const CalibStep y = calib_solve(sa, sb, sc, g0, g1, mu), z = calib_solve(sa, sb, sc, p0, p1, mu), w = calib_solve(sa, sb, sc, p0, p1, 0.0);
        x[0] = rec[(CF_IT + 8) * F + f];
        x[1] = ::fma(p0, z.n0 * z.id, p1 * (z.n1 * z.id));
        x[2] = rec[(CF_IT + 9) * F + f];
        x[3] = ::fma(p0, y.n0 * y.id, p1 * (y.n1 * y.id));
        x[4] = ::fma(p0, w.n0 * w.id, p1 * (w.n1 * w.id));
        x[5] = calib_det_ok(sa, sb, sc) ? 0.0 : 1.0;
    }, t2);
    const double Sd = t2[0];
    const double S = ::fma(1.0 + mu, Sd, t2[1]), R = t2[2] + t2[3], S0 = Sd + t2[4];
    if (status == -1 && moved) {
        if (free_len && !(S > ROVMPC_FIT_DET_MIN * (1.0 + mu) * Sd)) status = ROVMPC_FIT_DEGENERATE;
        else if (t2[5] != 0.0) status = ROVMPC_FIT_DEGENERATE;
    }
    if (status == -1 && iters >= a.max_iter) status = ROVMPC_FIT_MAX_ITER;
    if (status == -1 && mu > ROVMPC_CALIB_MU_MAX) status = ROVMPC_CALIB_STALLED;

    if (status == -1) {
        // (3) the next trial point of the group and of every frame
        const double dLn = free_len ? -R / S : 0.0;
        for (long long f = f0 + tid; f < f1; f += CALIB_RNT) {
            if (rec[CF_CLASS * F + f] != -1.0) continue;
            const double sa = rec[(CF_IT + 0) * F + f], sb = rec[(CF_IT + 1) * F + f], sc = rec[(CF_IT + 2) * F + f];
            const double th = rec[CF_TH * F + f], ga = rec[CF_GA * F + f];
            const CalibStep y = calib_solve(sa, sb, sc, rec[(CF_IT + 3) * F + f], rec[(CF_IT + 4) * F + f], mu);
            double dth = y.n0 * y.id, dga = y.n1 * y.id, tht, gat;
            if (free_len) {
                const CalibStep z = calib_solve(sa, sb, sc, rec[(CF_IT + 6) * F + f], rec[(CF_IT + 7) * F + f], mu);
                dth = ::fma(z.n0 * z.id, dLn, dth); dga = ::fma(z.n1 * z.id, dLn, dga);
                tht = th + dth; gat = ga + dga;
            } else {
                tht = ::fma(y.n0, y.id, th); gat = ::fma(y.n1, y.id, ga);   // the fit's trial point
            }
            rec[CF_THT * F + f] = tht;
            rec[CF_GAT * F + f] = gat;
            rec[CF_STEP * F + f] = ::fmax(::fabs(dth), ::fabs(dga));
        }
        if (tid == 0) {
            grp[CG_L] = L; grp[CG_LT] = L + dLn; grp[CG_DL] = dLn; grp[CG_MU] = mu; grp[CG_F] = Fg; grp[CG_F0] = F0;
            if (a.launch == 0) a.done[g] = 0;
        }
        return;
    }

    // (4) the group has ended: its row and its active frames' rows
    for (long long f = f0 + tid; f < f1; f += CALIB_RNT) {
        if (rec[CF_CLASS * F + f] != -1.0) continue;
        const double nw = rec[CF_NW * F + f];
        double *o = a.out_frame + ROVMPC_CALIB_FRAME_OUT * f;
        o[0] = rec[CF_TH * F + f]; o[1] = rec[CF_GA * F + f];
        o[2] = ::sqrt(rec[(CF_IT + 5) * F + f] / nw); o[3] = ::sqrt(rec[CF_F0 * F + f] / nw);
        o[4] = (double)status;
    }
    if (tid == 0) {
        const double dof = 3.0 * Nw - 2.0 * nact - 1.0, n = __builtin_nan("");
        double *o = a.out_group + (size_t)ROVMPC_CALIB_GROUP_OUT * g;
        o[0] = L;
        o[1] = nact > 0.0 ? ::sqrt(Fg / Nw) : n;
        o[2] = nact > 0.0 ? ::sqrt(F0 / Nw) : n;
        o[3] = free_len && nact > 0.0 && dof > 0.0 ? ::sqrt(Fg / dof / S0) : n;
        o[4] = (double)iters; o[5] = (double)status; o[6] = nact; o[7] = Nw;
        a.done[g] = 1;
    }
}

}  // namespace rovmpc
