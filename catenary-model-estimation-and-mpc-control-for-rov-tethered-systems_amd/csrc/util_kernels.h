// util_kernels.h -- batched mirrors of the reference's per-row helpers (fp64, gfx950).
// Each kernel replaces a Python loop of the reference; see include/rovmpc.h for the map.
#pragma once
#include "rollout_kernels.h"

namespace rovmpc {

// model.predict(X) on n already-scaled rows: one lane per row, operand stack in LDS.
__global__ void __launch_bounds__(256)
predict_kernel(const double *__restrict__ Xs, long long n, int F, const int32_t *code, int ncode,
               const double *consts, double *out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *stack = reinterpret_cast<double *>(smem_raw) + threadIdx.x;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = i < n ? i : n - 1;            // keep control flow uniform
    const double v = interp_eval<double>(code, ncode, consts, Xs + row * F, 1, stack, blockDim.x);
    if (i < n) out[i] = v;
}

// Forward integration of a Lagrangian's accelerations (evaluate_lagrangian_on_test.py:59-68), one lane per rollout:
//   a = dd(theta_{i-1}, gamma_{i-1}, v_{i-1});  v_i = v_{i-1} + a dt_i;  q_i = q_{i-1} + v_{i-1} dt_i,  dt_i = time[i] - time[i-1].
// out[4][B][T] = theta, gamma, vtheta, vgamma.  The two programs read features x0..x3 = (theta, gamma, vtheta, vgamma).
__global__ void __launch_bounds__(64)
lagrangian_rollout_kernel(const int32_t *code_th, int n_th, const int32_t *code_ga, int n_ga, const double *consts,
                          const double *__restrict__ time, long long T, const double *__restrict__ y0, long long B, double *out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int NT = blockDim.x;
    double *feat = reinterpret_cast<double *>(smem_raw) + threadIdx.x;          // [4][lane]
    double *stack = reinterpret_cast<double *>(smem_raw) + (size_t)4 * NT + threadIdx.x;
    const long long b0 = (long long)blockIdx.x * NT + threadIdx.x, b = b0 < B ? b0 : B - 1;   // uniform control flow
    double th = y0[4 * b], ga = y0[4 * b + 1], vt = y0[4 * b + 2], vg = y0[4 * b + 3];
    double *o_th = out + (size_t)b * T, *o_ga = out + ((size_t)B + b) * T, *o_vt = out + ((size_t)2 * B + b) * T,
           *o_vg = out + ((size_t)3 * B + b) * T;
    if (b0 < B) { o_th[0] = th; o_ga[0] = ga; o_vt[0] = vt; o_vg[0] = vg; }
    for (long long i = 1; i < T; ++i) {
        const double dt = time[i] - time[i - 1];                                                  // :60
        feat[0] = th; feat[NT] = ga; feat[2 * NT] = vt; feat[3 * NT] = vg;
        const double a_th = interp_eval<double>(code_th, n_th, consts, feat, NT, stack, NT);     // :61
        const double a_ga = interp_eval<double>(code_ga, n_ga, consts, feat, NT, stack, NT);     // :62
        const double vt_n = vt + a_th * dt, th_n = th + vt * dt;                                  // :64-65
        const double vg_n = vg + a_ga * dt, ga_n = ga + vg * dt;                                  // :67-68
        vt = vt_n; th = th_n; vg = vg_n; ga = ga_n;
        if (b0 < B) { o_th[i] = th; o_ga[i] = ga; o_vt[i] = vt; o_vg[i] = vg; }
    }
}

// The replay laws' arithmetic, shared by the replay kernels below and score_rows_kernel (score_kernels.h) so that the two
// cannot contract or associate differently: the increment of one first-order step and one step of the second-order chains.
// Where a product is fused into the sum that follows it is written out (contraction is off inside): the velocity update of
// the second-order laws is one fma, the angle update a rounded product and a sum -- what the replay kernels have always
// computed, now independent of the code around the call.
RV_DEV double replay_euler_increment(double k1, double dt) { return k1 * dt; }                   // main_fun.py:757-762
RV_DEV double replay_rk4_increment(double dt, double k1, double k2, double k4) {                  // simulate_rk4_theta_gamma.py:66
#pragma clang fp contract(off)
    return (dt / 6) * (k1 + 2 * k2 + 2 * k2 + k4);
}
// (y, v) <- one step over dt with dd0 = dd[i-1], dd1 = dd[i]
RV_DEV void replay_second_order_step(int integrator, double dd0, double dd1, double dt, double &y, double &v) {
#pragma clang fp contract(off)
    if (integrator == ROVMPC_DOUBLE_EULER) {
        y = y + v * dt;
        v = ::fma(dt, dd0, v);
    } else {
        v = ::fma(dt, (dd0 + dd1) / 2, v);
        y = y + dt * v;
    }
}

// Increments of rk4_integration (simulate_rk4_theta_gamma.py:56-66) / integrate_theta_gamma
// (main_fun.py:757-762) for step i = 1..T-1, both expressions.  inc[0] is unused.
__global__ void __launch_bounds__(128)
replay_increments_kernel(const double *__restrict__ Xs, const double *__restrict__ time, long long T, int F,
                         const int32_t *code_th, int n_th, const int32_t *code_ga, int n_ga,
                         const double *consts, int integrator, double *inc_th, double *inc_ga) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int NT = blockDim.x;
    double *feat = reinterpret_cast<double *>(smem_raw) + threadIdx.x;          // [F][lane]
    double *stack = reinterpret_cast<double *>(smem_raw) + (size_t)F * NT + threadIdx.x;
    const long long i0 = (long long)blockIdx.x * NT + threadIdx.x + 1;
    const long long i = i0 < T ? i0 : T - 1;
    const double dt = time[i] - time[i - 1];
    const double *x0 = Xs + (i - 1) * F, *x1 = Xs + i * F;
    double it, ig;
    {
        const double k1t = interp_eval<double>(code_th, n_th, consts, x0, 1, stack, NT);
        const double k1g = interp_eval<double>(code_ga, n_ga, consts, x0, 1, stack, NT);
        if (integrator == ROVMPC_EULER) {
            it = replay_euler_increment(k1t, dt); ig = replay_euler_increment(k1g, dt);
        } else {
            for (int f = 0; f < F; ++f) feat[(size_t)f * NT] = (x0[f] + x1[f]) / 2;   // :62-63
            const double k2t = interp_eval<double>(code_th, n_th, consts, feat, NT, stack, NT);
            const double k2g = interp_eval<double>(code_ga, n_ga, consts, feat, NT, stack, NT);
            const double k4t = interp_eval<double>(code_th, n_th, consts, x1, 1, stack, NT);
            const double k4g = interp_eval<double>(code_ga, n_ga, consts, x1, 1, stack, NT);
            it = replay_rk4_increment(dt, k1t, k2t, k4t);                             // :66
            ig = replay_rk4_increment(dt, k1g, k2g, k4g);
        }
    }
    if (i0 < T) { inc_th[i0] = it; inc_ga[i0] = ig; }
}

// Second-order replays: dd[i] = model.predict(X[i]) for every row (stored in inc_*), then
//   double Euler (test_cluster.py:110-129):  w[i] = w[i-1] + dd[i-1] dt_i ; y[i] = y[i-1] + w[i-1] dt_i
//   trapezoid   (dd_cluster.py:221-226):     w[i] = w[i-1] + (dd[i-1] + dd[i])/2 dt_i ; y[i] = y[i-1] + dt_i w[i]
// both from w[0] = 0, in the reference's sequential order; two lanes, one per series.
__global__ void __launch_bounds__(64)
replay_second_order_kernel(const double *dd_th, const double *dd_ga, const double *time, long long T, double th0,
                           double ga0, int integrator, double *th_out, double *ga_out) {
    const int w = threadIdx.x;
    if (w > 1) return;
    const double *dd = w == 0 ? dd_th : dd_ga;
    double *out = w == 0 ? th_out : ga_out;
    if (!out) return;
    double y = w == 0 ? th0 : ga0, v = 0.0;
    out[0] = y;
    for (long long i = 1; i < T; ++i) {
        const double dt = time[i] - time[i - 1];
        replay_second_order_step(integrator, dd[i - 1], dd[i], dt, y, v);
        out[i] = y;
    }
}

// y[i] = y[i-1] + inc[i] in the reference's (sequential) order; two lanes, one per series.
__global__ void __launch_bounds__(64)
replay_cumsum_kernel(const double *inc_th, const double *inc_ga, long long T, double th0, double ga0,
                     double *th_out, double *ga_out) {
    const int w = threadIdx.x;
    if (w > 1) return;
    const double *inc = w == 0 ? inc_th : inc_ga;
    double *out = w == 0 ? th_out : ga_out;
    if (!out) return;
    double y = w == 0 ? th0 : ga0;
    out[0] = y;
    for (long long i = 1; i < T; ++i) { y = y + inc[i]; out[i] = y; }
}

__global__ void __launch_bounds__(256)
solve_catenary_kernel(const double *l, const double *dH, double L, double c_lo, double c_hi,
                      double w_per_len, long long n, double *C_out, double *T_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CatRoot<double> c = solve_catenary_root<double>(l[i], dH[i], L, c_lo, c_hi);
    C_out[i] = c.C;
    if (T_out) T_out[i] = cable_tension<double>(l[i], c, w_per_len);
}

// main_fun.py:18-35 with the axis normalisation of :30.
RV_DEV V3<double> rodrigues_ref(V3<double> v, V3<double> axis, double ang) {
    const double inv = 1.0 / m_sqrt(dot3(axis, axis));
    const V3<double> k = {axis.x * inv, axis.y * inv, axis.z * inv};
    double s, c;
    m_sincos(ang, &s, &c);
    return rodrigues_unit(v, k, s, c);
}

__global__ void __launch_bounds__(256)
rodrigues_kernel(const double *v, const double *axis, const double *ang, long long n, double *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3<double> r = rodrigues_ref({v[3 * i], v[3 * i + 1], v[3 * i + 2]},
                                       {axis[3 * i], axis[3 * i + 1], axis[3 * i + 2]}, ang[i]);
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}

// Catenary(length=L)(a, b)[3]: M samples, uniform in the horizontal coordinate, of
// z = (cosh(C (x - x0)) - cosh(C x0)) / C in the vertical plane through a, b
// (catenary_model.py:10-12 shape law, C from main_fun.py:418-431).  Returns false when the
// reference's catenary_fn would return None at [3].
RV_DEV bool catenary_params(V3<double> rel, double L, double up, double c_lo, double c_hi,
                            double &l, double &C, double &x0, double &ch0) {
    l = m_sqrt(rel.x * rel.x + rel.y * rel.y);
    const double dH = up * rel.z;
    C = solve_catenary_C<double>(l, dH, L, c_lo, c_hi);
    if (!(C == C)) return false;
    x0 = 0.5 * l - m_atanh(dH / L) / C;
    ch0 = m_cosh(C * x0);
    return true;
}

RV_DEV V3<double> catenary_point(V3<double> a, V3<double> rel, double l, double C, double x0, double ch0,
                                 double up, int j, int M) {
    const double t = (double)j / (double)(M - 1);
    const double s = (m_cosh(C * (l * t - x0)) - ch0) / C;
    return {a.x + t * rel.x, a.y + t * rel.y, a.z + up * s};
}

__global__ void __launch_bounds__(256)
catenary_points_kernel(const double *A, const double *B, double L, double up, double c_lo, double c_hi,
                       long long n, int M, double *pts, int32_t *valid, double *params) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3<double> a = {A[3 * i], A[3 * i + 1], A[3 * i + 2]};
    const V3<double> rel = {B[3 * i] - a.x, B[3 * i + 1] - a.y, B[3 * i + 2] - a.z};
    double l, C, x0, ch0;
    const bool ok = catenary_params(rel, L, up, c_lo, c_hi, l, C, x0, ch0);
    valid[i] = ok ? 1 : 0;
    const double nan = m_nan<double>();
    if (params) {
        params[3 * i] = ok ? C : nan;
        params[3 * i + 1] = ok ? (ch0 - 1.0) / C : nan;
        params[3 * i + 2] = ok ? x0 : nan;
    }
    double *p = pts + (size_t)i * M * 3;
    for (int j = 0; j < M; ++j) {
        V3<double> q = ok ? catenary_point(a, rel, l, C, x0, ch0, up, j, M) : V3<double>{nan, nan, nan};
        p[3 * j] = q.x; p[3 * j + 1] = q.y; p[3 * j + 2] = q.z;
    }
}

// transform_catenary (main_fun.py:38-111) for n cases, one lane per case, the reference's
// two Rodrigues calls per point kept as they are (this is the full-shape path; the rollout
// kernel only needs the lowest z and uses the composed row instead).
__global__ void __launch_bounds__(128)
transform_catenary_kernel(const double *A, const double *B, const double *theta, const double *gamma,
                          double L, double up, double c_lo, double c_hi, long long n, int M,
                          double *out, int32_t *npts, double *z_low) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double nan = m_nan<double>();
    const V3<double> a = {A[3 * i], A[3 * i + 1], A[3 * i + 2]};
    const V3<double> b = {B[3 * i], B[3 * i + 1], B[3 * i + 2]};
    const V3<double> rel = {b.x - a.x, b.y - a.y, b.z - a.z};
    const double th = theta[i], ga = gamma[i];
    const size_t plane = (size_t)n * M * 3;
    double *o0 = out + (size_t)i * M * 3, *o1 = o0 + plane, *o2 = o1 + plane, *o3 = o2 + plane;
    auto put = [&](double *o, int j, V3<double> q) { o[3 * j] = q.x; o[3 * j + 1] = q.y; o[3 * j + 2] = q.z; };

    // Step 1: original catenary (:72)
    double l, C, x0, ch0;
    const bool ok0 = catenary_params(rel, L, up, c_lo, c_hi, l, C, x0, ch0);
    const int n0 = ok0 ? M : 2;
    for (int j = 0; j < M; ++j) {
        V3<double> q = {nan, nan, nan};
        if (ok0) q = catenary_point(a, rel, l, C, x0, ch0, up, j, M);
        else if (j == 0) q = a; else if (j == 1) q = b;
        put(o0, j, q);
    }
    // Step 2: axes (:75-89)
    V3<double> kt, kg;
    theta_gamma_axes<double>(rel, kt, kg);
    // Step 3: rotated end point and its catenary (:92-93)
    const V3<double> rb = rodrigues_ref(rel, kt, th);
    const V3<double> Bp = {a.x + rb.x, a.y + rb.y, a.z + rb.z};
    const bool ok1 = catenary_params(rb, L, up, c_lo, c_hi, l, C, x0, ch0);
    const int n1 = ok1 ? M : 2;
    double best = m_inf<double>();
    for (int j = 0; j < M; ++j) {
        V3<double> q = {nan, nan, nan}, q2 = q, q3 = q;
        if (j < n1) {
            if (ok1) q = catenary_point(a, rb, l, C, x0, ch0, up, j, M);
            else q = (j == 0) ? a : Bp;
            // Step 4 (:96-99) and Step 6 (:106-109)
            const V3<double> r2 = rodrigues_ref({q.x - a.x, q.y - a.y, q.z - a.z}, kt, -th);
            q2 = {a.x + r2.x, a.y + r2.y, a.z + r2.z};
            const V3<double> r3 = rodrigues_ref({q2.x - a.x, q2.y - a.y, q2.z - a.z}, kg, ga);
            q3 = {a.x + r3.x, a.y + r3.y, a.z + r3.z};
            const double zz = up * q3.z;
            best = (zz != zz) ? zz : (zz < best ? zz : best);
        }
        put(o1, j, q); put(o2, j, q2); put(o3, j, q3);
    }
    npts[2 * i] = n0; npts[2 * i + 1] = n1;
    if (z_low) z_low[i] = up * best;                      // fully_augmented_catenary.py:21-22
}

__global__ void __launch_bounds__(256)
velocity_transform_kernel(const double *R, const double *v, long long n, double *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = R + 9 * i, *u = v + 3 * i;
    out[3 * i] = r[0] * u[0] + r[1] * u[1] + r[2] * u[2];
    out[3 * i + 1] = r[3] * u[0] + r[4] * u[1] + r[5] * u[2];
    out[3 * i + 2] = r[6] * u[0] + r[7] * u[1] + r[8] * u[2];
}

// np.gradient(f, t) at row i of a length-T column with stride `ld` (numpy's non-uniform
// second-order interior formula, first-order one-sided edges; T == 1 is rejected by the host).
RV_DEV double np_gradient(const double *f, const double *t, long long i, long long T, int ld) {
    if (i == 0) return (f[ld] - f[0]) / (t[1] - t[0]);
    if (i == T - 1) return (f[(T - 1) * ld] - f[(T - 2) * ld]) / (t[T - 1] - t[T - 2]);
    const double dx1 = t[i] - t[i - 1], dx2 = t[i + 1] - t[i];
    const double a = -(dx2) / (dx1 * (dx1 + dx2)), b = (dx2 - dx1) / (dx1 * dx2), c = dx1 / (dx2 * (dx1 + dx2));
    return a * f[(i - 1) * ld] + b * f[i * ld] + c * f[(i + 1) * ld];
}

// extract_features (simply.py:15-41), one lane per row.
__global__ void __launch_bounds__(256)
extract_features_kernel(const double *__restrict__ P0, const double *__restrict__ P1, const double *__restrict__ V1,
                        const double *__restrict__ time, const double *__restrict__ theta,
                        const double *__restrict__ gamma, long long T, int with_prev, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int F = with_prev ? 18 : 16;
    double *o = out + i * F;
    const double *p1 = P1 + 3 * i, *p0 = P0 + 3 * i, *v = V1 + 3 * i;
    const double rx = p1[0] - p0[0], ry = p1[1] - p0[1], rz = p1[2] - p0[2];          // :25
    const double nr = m_sqrt(rx * rx + ry * ry + rz * rz);
    const double ux = rx / (nr + 1e-8), uy = ry / (nr + 1e-8), uz = rz / (nr + 1e-8);  // :26
    const double nv = m_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-8;           // :30
    o[0] = p1[0]; o[1] = p1[1]; o[2] = p1[2];
    o[3] = v[0]; o[4] = v[1]; o[5] = v[2];
    for (int a = 0; a < 3; ++a) o[6 + a] = np_gradient(V1 + a, time, i, T, 3);         // :20-23
    o[9] = ux; o[10] = uy; o[11] = uz;
    o[12] = m_clip(nr, 1e-5, 10.0);                                                     // :27
    o[13] = m_clip((v[0] * ux + v[1] * uy + v[2] * uz) / nv, -1.0, 1.0);                // :29-31
    o[14] = theta[i]; o[15] = gamma[i];
    if (with_prev) { o[16] = theta[i > 0 ? i - 1 : 0]; o[17] = gamma[i > 0 ? i - 1 : 0]; }   // :35-38
}

// features_dd (main_fun.py:811-871), pass 1 of 3, one lane per row.  W = window x window hat matrix of the
// Savitzky-Golay polynomial fit (host-built): interior rows use its centre row, the first / last half-window
// rows the polynomial fitted to the first / last `window` samples (scipy savgol_filter, mode='interp').
// Writes feature columns 0,1 (smoothed theta, gamma), 4,5 (v_sway, v_surge), 8..10 (V in m/s) of out[T][14].
__global__ void __launch_bounds__(256)
features_dd_pass1_kernel(const double *__restrict__ P0mm, const double *__restrict__ P1mm, const double *__restrict__ Vmm,
                         const double *__restrict__ theta, const double *__restrict__ gamma, const double *__restrict__ W,
                         int window, long long T, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int half = window / 2;
    long long first; int row;
    if (i < half) { first = 0; row = (int)i; }
    else if (i >= T - half) { first = T - window; row = (int)(i - first); }
    else { first = i - half; row = half; }
    const double *w = W + (size_t)row * window;
    double st = 0.0, sg = 0.0;
    for (int j = 0; j < window; ++j) { st += w[j] * theta[first + j]; sg += w[j] * gamma[first + j]; }
    double *o = out + i * 14;
    o[0] = st; o[1] = sg;                                                                    // :830-831
    const double vx = Vmm[3 * i] / 1000, vy = Vmm[3 * i + 1] / 1000, vz = Vmm[3 * i + 2] / 1000;   // :815
    const double rx = P1mm[3 * i] / 1000 - P0mm[3 * i] / 1000, ry = P1mm[3 * i + 1] / 1000 - P0mm[3 * i + 1] / 1000,
                 rz = P1mm[3 * i + 2] / 1000 - P0mm[3 * i + 2] / 1000;                       // :813-814, :839
    const double nr = m_sqrt(rx * rx + ry * ry + rz * rz) + 1e-8;                            // :841
    dd_surge_sway<double>(vx, vy, vz, rx / nr, ry / nr, rz / nr, o[4], o[5]);                // :842-843
    o[8] = vx; o[9] = vy; o[10] = vz;
}

// scipy.ndimage.gaussian_filter1d(x, sigma) (mode='reflect', truncate=4): symmetric FIR w[0..radius]
// (host-normalised), out[i] = w0 x[i] + sum_k w_k (x[i-k] + x[i+k]) with the edge sample repeated.
__global__ void __launch_bounds__(256)
gaussian_filter1d_kernel(const double *__restrict__ x, long long T, const double *__restrict__ w, int radius,
                         double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    auto at = [&](long long j) {
        while (j < 0 || j >= T) j = j < 0 ? -j - 1 : 2 * T - j - 1;      // d c b a | a b c d | d c b a
        return x[j];
    };
    double s = w[0] * x[i];
    for (int k = 1; k <= radius; ++k) s += w[k] * (at(i - k) + at(i + k));
    out[i] = s;
}

// passes 2 and 3: np.gradient of `npairs` columns of a [T][ld_src] table into columns of a [T][ld_dst] table.
__global__ void __launch_bounds__(256)
gradient_columns_kernel(const double *__restrict__ src, int ld_src, double *__restrict__ dst, int ld_dst,
                        const double *__restrict__ time, long long T, int npairs, const int *__restrict__ pairs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    for (int p = 0; p < npairs; ++p)
        dst[i * ld_dst + pairs[2 * p + 1]] = np_gradient(src + pairs[2 * p], time, i, T, ld_src);
}

// compute_rotation_kabsch (velocity_transform_batch.py:8-19) + the per-frame gates of :75-101,
// one lane per frame.  H = Pc^T Qc = U S V^T; R = V U^T with the reflection fix.  A proper
// rotation that maps u1 -> v1 and u2 -> v2 is unique, so R needs only the two dominant singular
// pairs: R = [v1 v2 v1xv2] [u1 u2 u1xu2]^T (this is what numpy's V^T-row flip produces, for any
// sign convention of the SVD, including the nearly planar marker sets a cable gives).
// The pairs come from one-sided Jacobi on the 3x3 H (column rotations until orthogonal).
__global__ void __launch_bounds__(128)
kabsch_kernel(const double *__restrict__ P, const double *__restrict__ Q, const double *__restrict__ v, long long T, int M,
              int batch_gates, double *v_out, double *R_out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const double nan = m_nan<double>();
    const double *p = P + (size_t)t * M * 3, *q = Q + (size_t)t * M * 3;
    double cp[3] = {0, 0, 0}, cq[3] = {0, 0, 0}, d2 = 0;
    bool finite = true;
    for (int i = 0; i < M; ++i)
        for (int a = 0; a < 3; ++a) {
            const double x = p[3 * i + a], y = q[3 * i + a];
            finite = finite && m_finite(x) && m_finite(y);
            cp[a] += x; cq[a] += y;
            d2 += (x - y) * (x - y);
        }
    bool ok = finite && M >= 3 && !(batch_gates && m_sqrt(d2) < 1e-6);
    double R[9];
    if (ok) {
        for (int a = 0; a < 3; ++a) { cp[a] /= M; cq[a] /= M; }
        double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};           // H[a][b] = sum_i Pc[i][a] Qc[i][b]
        for (int i = 0; i < M; ++i)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) A[a][b] += (p[3 * i + a] - cp[a]) * (q[3 * i + b] - cq[b]);
        // R does not depend on a scaling of H, but the squared column norms below overflow (and the columns divided by an
        // infinite norm are a finite zero matrix) or vanish once the markers are scaled far enough.  Bring the largest
        // magnitude of H into [0.5, 1) by its power of two: exact, so a frame the sweeps could already handle keeps its
        // bits.  An H that is not finite or all zero has no rotation: NaN row.
        double amax = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) { ok = ok && m_finite(A[a][b]); amax = m_abs(A[a][b]) > amax ? m_abs(A[a][b]) : amax; }
        ok = ok && amax > 0;
        int hexp = 0;
        ::frexp(ok ? amax : 1.0, &hexp);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) A[a][b] = ::ldexp(A[a][b], -hexp);
        double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int sweep = 0; sweep < 30; ++sweep) {
            bool rotated = false;
#pragma unroll
            for (int pair = 0; pair < 3; ++pair) {
                const int c0 = pair == 2 ? 1 : 0, c1 = pair == 0 ? 1 : 2;
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < 3; ++r) { al += A[r][c0] * A[r][c0]; be += A[r][c1] * A[r][c1]; ga += A[r][c0] * A[r][c1]; }
                if (m_abs(ga) > 1e-17 * m_sqrt(al * be) && ga != 0.0) {
                    const double zeta = (be - al) / (2 * ga);
                    const double tt = (zeta >= 0 ? 1.0 : -1.0) / (m_abs(zeta) + m_sqrt(1 + zeta * zeta));
                    const double c = 1.0 / m_sqrt(1 + tt * tt), s = c * tt;
                    for (int r = 0; r < 3; ++r) {
                        const double a0 = A[r][c0], a1 = A[r][c1];
                        A[r][c0] = c * a0 - s * a1; A[r][c1] = s * a0 + c * a1;
                        const double v0 = V[r][c0], v1 = V[r][c1];
                        V[r][c0] = c * v0 - s * v1; V[r][c1] = s * v0 + c * v1;
                    }
                    rotated = rotated || m_abs(ga) > 1e-15 * m_sqrt(al * be);
                }
            }
            if (!rotated) break;
        }
        // columns of A are sigma_j u_j, columns of V are v_j; take the two largest sigma
        double sg[3];
        for (int j = 0; j < 3; ++j) sg[j] = m_sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
        int j0 = 0;
        if (sg[1] > sg[j0]) j0 = 1;
        if (sg[2] > sg[j0]) j0 = 2;
        int j1 = j0 == 0 ? 1 : 0;
        for (int j = 0; j < 3; ++j) if (j != j0 && sg[j] > sg[j1]) j1 = j;
        V3<double> u1 = {A[0][j0] / sg[j0], A[1][j0] / sg[j0], A[2][j0] / sg[j0]};
        V3<double> u2 = {A[0][j1] / sg[j1], A[1][j1] / sg[j1], A[2][j1] / sg[j1]};
        const V3<double> v1 = {V[0][j0], V[1][j0], V[2][j0]}, v2 = {V[0][j1], V[1][j1], V[2][j1]};
        const V3<double> u3 = cross3(u1, u2), v3 = cross3(v1, v2);
        // R = V U^T = sum_j v_j u_j^T  (velocity_transform_batch.py:15)
        const double uu[3][3] = {{u1.x, u1.y, u1.z}, {u2.x, u2.y, u2.z}, {u3.x, u3.y, u3.z}};
        const double vv[3][3] = {{v1.x, v1.y, v1.z}, {v2.x, v2.y, v2.z}, {v3.x, v3.y, v3.z}};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) R[3 * a + b] = vv[0][a] * uu[0][b] + vv[1][a] * uu[1][b] + vv[2][a] * uu[2][b];
        // A rank-one H (collinear markers) determines no rotation.  The sweeps then leave a residual column parallel to the
        // dominant one, u2 = +-u1 and R is a finite matrix of rank one -- unless the residual happens to underflow first.
        // So the result itself is gated, as the reference's batch loop gates its own (:94, there to 1e-2): a frame
        // whose R is not orthogonal to 32 eps is a NaN row.  Converged sweeps leave |u1.u2| <= 1e-15 and a defect of a
        // few eps; det R = +1 follows from the cross products once R is orthogonal.
        double defect = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                const double s = R[3 * a] * R[3 * b] + R[3 * a + 1] * R[3 * b + 1] + R[3 * a + 2] * R[3 * b + 2] - (a == b ? 1.0 : 0.0);
                defect = m_abs(s) > defect || s != s ? m_abs(s) : defect;
            }
        ok = ok && defect <= 32 * m_eps<double>();
    }
    const double *w = v + 3 * t;
    for (int a = 0; a < 3; ++a)
        v_out[3 * t + a] = ok ? R[3 * a] * w[0] + R[3 * a + 1] * w[1] + R[3 * a + 2] * w[2] : nan;   // :100-101
    if (R_out) for (int a = 0; a < 9; ++a) R_out[9 * t + a] = ok ? R[a] : nan;
}

// compute_catenary_3D(p0, p1, rope_length, num_points) (models/catenary_3d.py:5-39) -- the catenary generator the reference
// itself holds (pympc's is absent): straight np.linspace when the rope is not longer than the distance (:13-14), otherwise
// the fixed point a <- a L / (2 a sinh(d / 2a)) from a = d / 2, at most 100 rounds, stop when |a_new - a| < 1e-6 (:18-24),
// and z lowered by a cosh(half_span / a) - a cosh(x / a) along the chord (:26-37).  One lane per pair, the reference's own
// operation order (no contraction: its NumPy evaluates every product and sum separately).  a_out[i] = NaN for the straight case.
// (The update multiplies a by L / arc(a) > 1 while the rope is longer than the arc, i.e. it walks AWAY from the hanging
// solution and normally spends all 100 rounds: the curve it returns is nearly flat, its sag the difference of two numbers
// of size a ~ 1e6..1e30 -- rounding noise in multiples of ulp(a).  Reproduced as it is; parity with the host's libm can
// therefore only be asked to a few ulp of a cosh(half / a), and the tests ask exactly that.)
__global__ void __launch_bounds__(128)
catenary_3d_kernel(const double *P0, const double *P1, double rope, long long n, int M, double *pts, double *a_out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x0 = P0[3 * i], y0 = P0[3 * i + 1], z0 = P0[3 * i + 2];
    const double x1 = P1[3 * i], y1 = P1[3 * i + 1], z1 = P1[3 * i + 2];
    const double dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
    const double direct = ::sqrt((dx * dx + dy * dy) + dz * dz);
    double *p = pts + (size_t)i * M * 3;
    if (rope <= direct || !(direct == direct)) {
        // np.linspace(p0, p1, M): start + j * step, the last sample set to the stop value (a NaN distance has no `<=`, so the
        // reference would go on and produce NaN; so does this branch)
        const double sx = dx / (double)(M - 1), sy = dy / (double)(M - 1), sz = dz / (double)(M - 1);
        for (int j = 0; j < M; ++j) {
            const bool last = j == M - 1;
            p[3 * j] = last ? x1 : x0 + (double)j * sx;
            p[3 * j + 1] = last ? y1 : y0 + (double)j * sy;
            p[3 * j + 2] = last ? z1 : z0 + (double)j * sz;
        }
        if (a_out) a_out[i] = m_nan<double>();
        return;
    }
    const double half = direct / 2.0;
    double a = half;
    for (int it = 0; it < 100; ++it) {
        const double lhs = 2.0 * a * ::sinh(direct / (2.0 * a));
        const double a_new = a * rope / lhs;
        const bool done = ::fabs(a_new - a) < 1e-6;
        a = a_new;
        if (done) break;
    }
    const double off = a * ::cosh(half / a);
    for (int j = 0; j < M; ++j) {
        const double t = (double)j / (double)(M - 1);
        const double x_pos = t * direct - half;
        const double sag = off - a * ::cosh(x_pos / a);
        p[3 * j] = x0 + dx * t;
        p[3 * j + 1] = y0 + dy * t;
        p[3 * j + 2] = (z0 + dz * t) - sag;
    }
    if (a_out) a_out[i] = a;
}

// ---- rovmpc_math_probe: one primitive of device_math.h by itself (diagnostic) --------------------------------------------
// Element i on global thread i of 256-thread blocks: elements 64 w .. 64 w + 63 are the lanes of wave w, which is what
// decides the wave-uniform large-argument branch of the trig kernels.  The functions are called as the kernels call them;
// fn is uniform over the launch.  Threads past n leave before the call, so the last wave runs with a partial exec mask.
template <typename T>
__global__ void __launch_bounds__(256)
math_probe_kernel(int fn, const T *__restrict__ x, const T *__restrict__ y, long long n, T *__restrict__ out0, T *__restrict__ out1) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T a = x[i], b = y ? y[i] : T(0);
    T r0 = T(0), r1 = T(0);
    switch (fn) {
        case ROVMPC_PROBE_SIN: r0 = m_sin(a); break;
        case ROVMPC_PROBE_SIN_PINNED: { const Trig<T> tg(true); r0 = tg.sin(a); break; }
        case ROVMPC_PROBE_SIN_BOUNDED: { const Trig<T> tg(true); r0 = tg.sin_bounded(a); break; }
        case ROVMPC_PROBE_SINCOS: m_sincos(a, &r0, &r1); break;
        case ROVMPC_PROBE_SINCOS_PINNED: { const Trig<T> tg(true); tg.sincos(a, &r0, &r1); break; }
        case ROVMPC_PROBE_RCP: r0 = fast_rcp(a); break;
        case ROVMPC_PROBE_DIV: r0 = m_div(a, b); break;
        case ROVMPC_PROBE_DIVQ: r0 = m_divq(a, b); break;
        case ROVMPC_PROBE_DIVX: r0 = m_divx(a, b); break;
        case ROVMPC_PROBE_SQRTQ: r0 = m_sqrtq(a); break;
        case ROVMPC_PROBE_SQRT: r0 = m_sqrt(a); break;
        case ROVMPC_PROBE_MIN_RAW: r0 = m_min_raw(a, b); break;
        case ROVMPC_PROBE_EXP_INC: r0 = exp_increment(a); break;
        case ROVMPC_PROBE_EXP_INC_TINY: r0 = exp_increment_tiny(a); break;
        case ROVMPC_PROBE_SINH_POS: r0 = sinh_pos(a); break;
        case ROVMPC_PROBE_SINHC_M1_SMALL: r0 = sinhc_m1_small(a); break;
        case ROVMPC_PROBE_COSH_M1_SMALL: r0 = cosh_m1_small(a); break;
        default: break;
    }
    out0[i] = r0;
    if (out1) out1[i] = r1;
}

}  // namespace rovmpc
