// helpers_host.hip -- the batched helper entries of include/rovmpc.h: host pointers in, host pointers out.
#include "rovmpc_internal.h"

#include "util_kernels.h"
#include "fit_kernels.h"
#include "calib_kernels.h"
#include "track_kernels.h"
#include "score_kernels.h"
#include "refit_kernels.h"
#include "discover_kernels.h"
#include "horizon_kernels.h"

// ---- batched helper mirrors (host pointers, fp64) ---------------------------------------------

namespace {          // (the scaffold's types stay out of the library's dynamic symbols)

// n elements of T in device memory, owned by the HelperCall that handed it out.
template <typename T> struct DevArray {
    T *p; size_t n;
    operator T *() const { return p; }
};

// One helper call.  Sets the device, hands out device buffers that it frees on every exit path, queues uploads and copies
// back on h->stream, and finish() ends the call with the launch check and one synchronise.  The first HIP error is kept:
// every later step of the scaffold does nothing, the entry skips its launches (ok()), and finish() reports that error.
class HelperCall {
    rovmpc_handle *h_;
    std::vector<void *> owned_;
    hipError_t err_ = hipSuccess;
    const char *what_ = "";
    int line_ = 0;
    bool keep(hipError_t e, const char *what, int line) {
        if (err_ == hipSuccess && e != hipSuccess) { err_ = e; what_ = what; line_ = line; }
        return err_ == hipSuccess;
    }
    void *alloc(size_t bytes) {          // (never zero bytes: an empty optional input still gets a pointer)
        void *p = nullptr;
        if (ok() && keep(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc", __LINE__)) owned_.push_back(p);
        return p;
    }
    void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        if (ok()) keep(hipMemcpyAsync(dst, src, bytes, kind, h_->stream), "hipMemcpyAsync", __LINE__);
    }
public:
    explicit HelperCall(rovmpc_handle *h) : h_(h) { keep(hipSetDevice(h->cfg.device), "hipSetDevice", __LINE__); }
    ~HelperCall() { for (void *p : owned_) (void)hipFree(p); }
    HelperCall(const HelperCall &) = delete;
    HelperCall &operator=(const HelperCall &) = delete;
    bool ok() const { return err_ == hipSuccess; }
    template <typename T> DevArray<T> buffer(size_t n) { return {(T *)alloc(n * sizeof(T)), n}; }
    template <typename T> DevArray<T> upload(const T *src, size_t n) {
        DevArray<T> d = buffer<T>(n);
        copy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    // the whole buffer back to the host; a null `dst` is an optional output the caller did not ask for
    template <typename T> void download(T *dst, const DevArray<T> &d) {
        if (dst) copy(dst, d.p, d.n * sizeof(T), hipMemcpyDeviceToHost);
    }
    int finish() {
        if (ok()) keep(hipGetLastError(), "hipGetLastError()", __LINE__);
        if (ok()) keep(hipStreamSynchronize(h_->stream), "hipStreamSynchronize(h->stream)", __LINE__);
        if (ok()) return ROVMPC_OK;
        FAIL(h_, ROVMPC_ERR_HIP, "%s failed: %s (%s:%d)", what_, hipGetErrorString(err_), __FILE__, line_);
    }
};

}  // namespace

static inline int grid_for(long long n, int bs) { return (int)((n + bs - 1) / bs); }

extern "C" int rovmpc_predict(rovmpc_handle *h, const double *Xs, int64_t n, int32_t which, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!h->has_model) FAIL(h, ROVMPC_ERR_NO_MODEL, "rovmpc_set_model has not been called");
    if (n < 0 || (n > 0 && (!Xs || !out)) || which < 0 || which > 1) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_predict: bad argument");
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dX = c.upload(Xs, (size_t)n * h->n_feat);
    const auto dO = c.buffer<double>((size_t)n);
    const int bs = 256;
    if (c.ok())
        hipLaunchKernelGGL(predict_kernel, dim3(grid_for(n, bs)), dim3(bs), ROVMPC_MAX_STACK * bs * sizeof(double), h->stream,
                           dX.p, (long long)n, h->n_feat, which == 0 ? h->d_code_th : h->d_code_ga,
                           which == 0 ? h->n_th : h->n_ga, h->d_consts64, dO.p);
    c.download(out, dO);
    return c.finish();
}

extern "C" int rovmpc_eval_expression(rovmpc_handle *h, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts,
                                      const double *X, int32_t F, int64_t n, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!code || n < 0 || F < 1 || F > ROVMPC_MAX_FEATURES || n_consts < 0 || n_consts > ROVMPC_MAX_CODE || (n_consts > 0 && !consts) ||
        (n > 0 && (!X || !out)))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_eval_expression: bad argument");
    if (const char *why = validate_code(code, n_code, F, n_consts)) FAIL(h, ROVMPC_ERR_INVALID, "program: %s", why);
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const double zero = 0.0;
    const auto dX = c.upload(X, (size_t)n * F);
    const auto dC = c.upload(code, (size_t)n_code);
    const auto dK = c.upload(n_consts ? consts : &zero, (size_t)(n_consts ? n_consts : 1));
    const auto dO = c.buffer<double>((size_t)n);
    const int bs = 256;
    if (c.ok())
        hipLaunchKernelGGL(predict_kernel, dim3(grid_for(n, bs)), dim3(bs), ROVMPC_MAX_STACK * bs * sizeof(double), h->stream,
                           dX.p, (long long)n, (int)F, dC.p, (int)n_code, dK.p, dO.p);
    c.download(out, dO);
    return c.finish();
}

template <typename T>
static int math_probe_run(rovmpc_handle *h, int32_t fn, const double *x, const double *y, int64_t n, double *out0, double *out1) {
    std::vector<T> hx(x, x + n), hy, ho((size_t)n), ho1;          // (plain conversion to T)
    if (y) hy.assign(y, y + n);
    if (out1) ho1.resize((size_t)n);
    HelperCall c(h);
    const auto dX = c.upload(hx.data(), (size_t)n);
    const auto dY = y ? c.upload(hy.data(), (size_t)n) : DevArray<T>{nullptr, 0};
    const auto dO = c.buffer<T>((size_t)n);
    const auto dO1 = out1 ? c.buffer<T>((size_t)n) : DevArray<T>{nullptr, 0};
    if (c.ok())
        hipLaunchKernelGGL(math_probe_kernel<T>, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, (int)fn, (const T *)dX.p,
                           (const T *)dY.p, (long long)n, dO.p, dO1.p);
    c.download(ho.data(), dO);
    if (out1) c.download(ho1.data(), dO1);
    if (int rc = c.finish()) return rc;
    for (int64_t i = 0; i < n; ++i) out0[i] = (double)ho[i];
    if (out1) for (int64_t i = 0; i < n; ++i) out1[i] = (double)ho1[i];
    return ROVMPC_OK;
}

extern "C" int rovmpc_math_probe(rovmpc_handle *h, int32_t fn, int32_t dtype, const double *x, const double *y, int64_t n,
                                 double *out0, double *out1) {
    if (!h) return ROVMPC_ERR_INVALID;
    const bool two_in = fn == ROVMPC_PROBE_DIV || fn == ROVMPC_PROBE_DIVQ || fn == ROVMPC_PROBE_DIVX || fn == ROVMPC_PROBE_MIN_RAW;
    if (fn < 0 || fn >= ROVMPC_PROBE_COUNT || (dtype != ROVMPC_F64 && dtype != ROVMPC_F32) || n < 0 || n > (int64_t)1 << 24 ||
        (n > 0 && (!x || !out0 || (two_in && !y))))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_math_probe: bad argument");
    if (fn == ROVMPC_PROBE_SIN_BOUNDED)                      // the unchecked sine is undefined outside its limit
        for (int64_t i = 0; i < n; ++i) {
            const double v = dtype == ROVMPC_F32 ? (double)(float)x[i] : x[i];
            if (!(fabs(v) < (dtype == ROVMPC_F32 ? (double)TRIGF_FAST_LIMIT : TRIG_FAST_LIMIT)))
                FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_math_probe: input %lld (%g) is outside the bounded sine's domain", (long long)i, x[i]);
        }
    if (n == 0) return ROVMPC_OK;
    if (!two_in) y = nullptr;
    return dtype == ROVMPC_F32 ? math_probe_run<float>(h, fn, x, y, n, out0, out1) : math_probe_run<double>(h, fn, x, y, n, out0, out1);
}

extern "C" int rovmpc_lagrangian_rollout(rovmpc_handle *h, const int32_t *code_th, int32_t n_th, const int32_t *code_ga, int32_t n_ga,
                                         const double *consts, int32_t n_consts, const double *time, int64_t T, const double *y0,
                                         int64_t B, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!code_th || !code_ga || !time || !y0 || !out || T < 1 || B < 1 || n_consts < 0 || n_consts > ROVMPC_MAX_CODE || (n_consts > 0 && !consts))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_lagrangian_rollout: bad argument");
    const char *why;
    if ((why = validate_code(code_th, n_th, 4, n_consts))) FAIL(h, ROVMPC_ERR_INVALID, "theta acceleration program: %s", why);
    if ((why = validate_code(code_ga, n_ga, 4, n_consts))) FAIL(h, ROVMPC_ERR_INVALID, "gamma acceleration program: %s", why);
    HelperCall c(h);
    const double zero = 0.0;
    const auto dCt = c.upload(code_th, (size_t)n_th);
    const auto dCg = c.upload(code_ga, (size_t)n_ga);
    const auto dK = c.upload(n_consts ? consts : &zero, (size_t)(n_consts ? n_consts : 1));
    const auto dT = c.upload(time, (size_t)T);
    const auto dY = c.upload(y0, (size_t)B * 4);
    const auto dO = c.buffer<double>((size_t)4 * B * T);
    const int bs = 64;
    if (c.ok())
        hipLaunchKernelGGL(lagrangian_rollout_kernel, dim3(grid_for(B, bs)), dim3(bs), (size_t)(4 + ROVMPC_MAX_STACK) * bs * sizeof(double), h->stream,
                           dCt.p, (int)n_th, dCg.p, (int)n_ga, dK.p, dT.p, (long long)T, dY.p, (long long)B, dO.p);
    c.download(out, dO);
    return c.finish();
}

extern "C" int rovmpc_replay(rovmpc_handle *h, const double *Xs, const double *time, int64_t T, double theta0, double gamma0,
                             int32_t integrator, double *theta_out, double *gamma_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!h->has_model) FAIL(h, ROVMPC_ERR_NO_MODEL, "rovmpc_set_model has not been called");
    if (T < 1 || !Xs || !time || integrator < ROVMPC_RK4 || integrator > ROVMPC_TRAPEZOID)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_replay: bad argument");
    HelperCall c(h);
    const auto dX = c.upload(Xs, (size_t)T * h->n_feat);
    const auto dT = c.upload(time, (size_t)T);
    const auto dIt = c.buffer<double>((size_t)T), dIg = c.buffer<double>((size_t)T);
    const auto dOt = c.buffer<double>((size_t)T), dOg = c.buffer<double>((size_t)T);
    if (!c.ok()) return c.finish();
    if (integrator >= ROVMPC_DOUBLE_EULER) {
        // second-derivative models: predict every row, then integrate twice
        const int bs = 256;
        for (int which = 0; which < 2; ++which)
            hipLaunchKernelGGL(predict_kernel, dim3(grid_for(T, bs)), dim3(bs), ROVMPC_MAX_STACK * bs * sizeof(double), h->stream,
                               dX.p, (long long)T, h->n_feat, which == 0 ? h->d_code_th : h->d_code_ga,
                               which == 0 ? h->n_th : h->n_ga, h->d_consts64, which == 0 ? dIt.p : dIg.p);
        hipLaunchKernelGGL(replay_second_order_kernel, dim3(1), dim3(64), 0, h->stream, dIt.p, dIg.p, dT.p, (long long)T, theta0,
                           gamma0, integrator, dOt.p, dOg.p);
    } else {
        if (T > 1) {
            const int bs = 128;
            const size_t lds = (size_t)(h->n_feat + ROVMPC_MAX_STACK) * bs * sizeof(double);
            hipLaunchKernelGGL(replay_increments_kernel, dim3(grid_for(T - 1, bs)), dim3(bs), lds, h->stream, dX.p, dT.p,
                               (long long)T, h->n_feat, h->d_code_th, h->n_th, h->d_code_ga, h->n_ga, h->d_consts64, integrator,
                               dIt.p, dIg.p);
        }
        hipLaunchKernelGGL(replay_cumsum_kernel, dim3(1), dim3(64), 0, h->stream, dIt.p, dIg.p, (long long)T, theta0, gamma0,
                           dOt.p, dOg.p);
    }
    c.download(theta_out, dOt);
    c.download(gamma_out, dOg);
    return c.finish();
}

extern "C" int rovmpc_solve_catenary(rovmpc_handle *h, const double *l, const double *dH, double L, int64_t n, double *C_out,
                                     double *T_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (n < 0 || (n > 0 && (!l || !dH || !C_out))) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_solve_catenary: bad argument");
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dl = c.upload(l, (size_t)n);
    const auto dh = c.upload(dH, (size_t)n);
    const auto dC = c.buffer<double>((size_t)n), dT = c.buffer<double>((size_t)n);
    if (c.ok())
        hipLaunchKernelGGL(solve_catenary_kernel, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, dl.p, dh.p, L, h->cfg.c_lo,
                           h->cfg.c_hi, h->cfg.cable_wet_weight / L, (long long)n, dC.p, T_out ? dT.p : nullptr);
    c.download(C_out, dC);
    c.download(T_out, dT);
    return c.finish();
}

extern "C" int rovmpc_rodrigues(rovmpc_handle *h, const double *v, const double *axis, const double *angle, int64_t n, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (n < 0 || (n > 0 && (!v || !axis || !angle || !out))) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_rodrigues: bad argument");
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dv = c.upload(v, (size_t)n * 3);
    const auto da = c.upload(axis, (size_t)n * 3);
    const auto dg = c.upload(angle, (size_t)n);
    const auto dout = c.buffer<double>((size_t)n * 3);
    if (c.ok())
        hipLaunchKernelGGL(rodrigues_kernel, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, dv.p, da.p, dg.p, (long long)n, dout.p);
    c.download(out, dout);
    return c.finish();
}

extern "C" int rovmpc_catenary_points(rovmpc_handle *h, const double *A, const double *B, double L, int64_t n, int32_t M,
                                      double *pts, int32_t *valid, double *params) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (n < 0 || M < 2 || (n > 0 && (!A || !B || !pts || !valid))) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_catenary_points: bad argument");
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dA = c.upload(A, (size_t)n * 3);
    const auto dB = c.upload(B, (size_t)n * 3);
    const auto dP = c.buffer<double>((size_t)n * M * 3);
    const auto dV = c.buffer<int32_t>((size_t)n);
    const auto dQ = c.buffer<double>((size_t)n * 3);
    const double up = h->cfg.frame == ROVMPC_ENU ? 1.0 : -1.0;
    if (c.ok())
        hipLaunchKernelGGL(catenary_points_kernel, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, dA.p, dB.p, L, up, h->cfg.c_lo,
                           h->cfg.c_hi, (long long)n, M, dP.p, dV.p, dQ.p);
    c.download(pts, dP);
    c.download(valid, dV);
    c.download(params, dQ);
    return c.finish();
}

extern "C" int rovmpc_compute_catenary_3d(rovmpc_handle *h, const double *p0, const double *p1, double rope_length, int64_t n,
                                          int32_t num_points, double *pts, double *a_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (n < 0 || num_points < 2 || (n > 0 && (!p0 || !p1 || !pts))) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_compute_catenary_3d: bad argument");
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dA = c.upload(p0, (size_t)n * 3);
    const auto dB = c.upload(p1, (size_t)n * 3);
    const auto dP = c.buffer<double>((size_t)n * num_points * 3);
    const auto dQ = c.buffer<double>((size_t)n);
    if (c.ok())
        hipLaunchKernelGGL(catenary_3d_kernel, dim3(grid_for(n, 128)), dim3(128), 0, h->stream, dA.p, dB.p, rope_length,
                           (long long)n, num_points, dP.p, dQ.p);
    c.download(pts, dP);
    c.download(a_out, dQ);
    return c.finish();
}

extern "C" int rovmpc_transform_catenary(rovmpc_handle *h, const double *A, const double *B, const double *theta,
                                         const double *gamma, double L, int64_t n, int32_t M, double *out, int32_t *npts,
                                         double *z_low) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (n < 0 || M < 2 || (n > 0 && (!A || !B || !theta || !gamma || !out || !npts)))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_transform_catenary: bad argument");
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dA = c.upload(A, (size_t)n * 3);
    const auto dB = c.upload(B, (size_t)n * 3);
    const auto dt = c.upload(theta, (size_t)n);
    const auto dg = c.upload(gamma, (size_t)n);
    const auto dO = c.buffer<double>((size_t)4 * n * M * 3);
    const auto dN = c.buffer<int32_t>((size_t)n * 2);
    const auto dZ = c.buffer<double>((size_t)n);
    const double up = h->cfg.frame == ROVMPC_ENU ? 1.0 : -1.0;
    if (c.ok())
        hipLaunchKernelGGL(transform_catenary_kernel, dim3(grid_for(n, 128)), dim3(128), 0, h->stream, dA.p, dB.p, dt.p, dg.p, L, up,
                           h->cfg.c_lo, h->cfg.c_hi, (long long)n, M, dO.p, dN.p, dZ.p);
    c.download(out, dO);
    c.download(npts, dN);
    c.download(z_low, dZ);
    return c.finish();
}

extern "C" int rovmpc_velocity_transform(rovmpc_handle *h, const double *R, const double *v, int64_t n, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (n < 0 || (n > 0 && (!R || !v || !out))) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_velocity_transform: bad argument");
    if (n == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dR = c.upload(R, (size_t)n * 9);
    const auto dv = c.upload(v, (size_t)n * 3);
    const auto dout = c.buffer<double>((size_t)n * 3);
    if (c.ok())
        hipLaunchKernelGGL(velocity_transform_kernel, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, dR.p, dv.p, (long long)n, dout.p);
    c.download(out, dout);
    return c.finish();
}

extern "C" int rovmpc_extract_features(rovmpc_handle *h, const double *P0, const double *P1, const double *V1, const double *time,
                                       const double *theta, const double *gamma, int64_t T, int32_t with_prev, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (T < 2 || !P0 || !P1 || !V1 || !time || !theta || !gamma || !out)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_extract_features: bad argument (np.gradient needs at least 2 rows)");
    HelperCall c(h);
    const int F = with_prev ? 18 : 16;
    const auto d0 = c.upload(P0, (size_t)T * 3);
    const auto d1 = c.upload(P1, (size_t)T * 3);
    const auto dv = c.upload(V1, (size_t)T * 3);
    const auto dt = c.upload(time, (size_t)T);
    const auto dth = c.upload(theta, (size_t)T);
    const auto dga = c.upload(gamma, (size_t)T);
    const auto dout = c.buffer<double>((size_t)T * F);
    if (c.ok())
        hipLaunchKernelGGL(extract_features_kernel, dim3(grid_for(T, 256)), dim3(256), 0, h->stream, d0.p, d1.p, dv.p, dt.p, dth.p,
                           dga.p, (long long)T, with_prev, dout.p);
    c.download(out, dout);
    return c.finish();
}

// Hat matrix of the least-squares polynomial fit of degree `order` on `window` equally spaced samples
// (centred abscissae): H = Q Q^T with Q the orthonormalised monomials (modified Gram-Schmidt, twice).
static void savgol_hat_matrix(int window, int order, std::vector<double> &H) {
    const int w = window, m = order + 1, half = w / 2;
    std::vector<long double> Q((size_t)w * m);
    for (int c = 0; c < m; ++c) {
        for (int r = 0; r < w; ++r) Q[(size_t)r * m + c] = powl((long double)(r - half), c);
        for (int pass = 0; pass < 2; ++pass)
            for (int p = 0; p < c; ++p) {
                long double d = 0;
                for (int r = 0; r < w; ++r) d += Q[(size_t)r * m + c] * Q[(size_t)r * m + p];
                for (int r = 0; r < w; ++r) Q[(size_t)r * m + c] -= d * Q[(size_t)r * m + p];
            }
        long double n = 0;
        for (int r = 0; r < w; ++r) n += Q[(size_t)r * m + c] * Q[(size_t)r * m + c];
        n = sqrtl(n);
        for (int r = 0; r < w; ++r) Q[(size_t)r * m + c] /= n;
    }
    H.assign((size_t)w * w, 0.0);
    for (int i = 0; i < w; ++i)
        for (int j = 0; j < w; ++j) {
            long double s = 0;
            for (int c = 0; c < m; ++c) s += Q[(size_t)i * m + c] * Q[(size_t)j * m + c];
            H[(size_t)i * w + j] = (double)s;
        }
}

extern "C" int rovmpc_features_dd(rovmpc_handle *h, const double *P0_mm, const double *P1_mm, const double *V_mm, const double *time,
                                  const double *theta, const double *gamma, int64_t T, int32_t window, int32_t polyorder,
                                  double *features, double *targets) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!P0_mm || !P1_mm || !V_mm || !time || !theta || !gamma || !features)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_features_dd: null argument");
    if (window < 3 || window > 255 || window % 2 == 0 || polyorder < 0 || polyorder >= window)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_features_dd: window must be odd in 3..255 and polyorder < window (got %d, %d)", window, polyorder);
    if (T < window) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_features_dd: %lld rows, fewer than the smoothing window %d (savgol_filter mode='interp')", (long long)T, window);
    std::vector<double> H;
    savgol_hat_matrix(window, polyorder, H);
    HelperCall c(h);
    const auto d0 = c.upload(P0_mm, (size_t)T * 3);
    const auto d1 = c.upload(P1_mm, (size_t)T * 3);
    const auto dv = c.upload(V_mm, (size_t)T * 3);
    const auto dt = c.upload(time, (size_t)T);
    const auto dth = c.upload(theta, (size_t)T);
    const auto dga = c.upload(gamma, (size_t)T);
    const auto dW = c.upload((const double *)H.data(), H.size());
    // pass 2: [dtheta, dgamma, a_sway, a_surge, a_x, a_y, a_z] <- gradients of pass-1 columns (main_fun.py:825-847);
    // pass 3: targets [ddtheta, ddgamma] <- gradients of columns 2, 3 (:835-836)
    const int pairs[] = {0, 2, 1, 3, 4, 6, 5, 7, 8, 11, 9, 12, 10, 13, /* pass 3 */ 2, 0, 3, 1};
    const auto dpairs = c.upload(pairs, sizeof(pairs) / sizeof(pairs[0]));
    const auto dF = c.buffer<double>((size_t)T * 14);
    const auto dY = c.buffer<double>((size_t)T * 2);
    const dim3 grid(grid_for(T, 256)), block(256);
    if (c.ok()) {
        hipLaunchKernelGGL(features_dd_pass1_kernel, grid, block, 0, h->stream, d0.p, d1.p, dv.p, dth.p, dga.p, dW.p, window,
                           (long long)T, dF.p);
        hipLaunchKernelGGL(gradient_columns_kernel, grid, block, 0, h->stream, (const double *)dF.p, 14, dF.p, 14, dt.p,
                           (long long)T, 7, (const int *)dpairs.p);
        hipLaunchKernelGGL(gradient_columns_kernel, grid, block, 0, h->stream, (const double *)dF.p, 14, dY.p, 2, dt.p,
                           (long long)T, 2, (const int *)dpairs.p + 14);
    }
    c.download(features, dF);
    c.download(targets, dY);
    return c.finish();
}

extern "C" int rovmpc_gaussian_filter1d(rovmpc_handle *h, const double *x, int64_t T, double sigma, double truncate, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (T < 1 || !x || !out || !(sigma > 0) || !(truncate > 0))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_gaussian_filter1d: bad argument");
    const int radius = (int)(truncate * sigma + 0.5);                  // scipy/ndimage/_filters.py gaussian_filter1d
    if (radius > 4096) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_gaussian_filter1d: kernel radius %d too large", radius);
    std::vector<double> w(radius + 1);
    double sum = 0.0;
    for (int k = -radius; k <= radius; ++k) sum += exp(-0.5 / (sigma * sigma) * (double)k * (double)k);
    for (int k = 0; k <= radius; ++k) w[k] = exp(-0.5 / (sigma * sigma) * (double)k * (double)k) / sum;
    HelperCall c(h);
    const auto dx = c.upload(x, (size_t)T);
    const auto dw = c.upload((const double *)w.data(), w.size());
    const auto dout = c.buffer<double>((size_t)T);
    if (c.ok())
        hipLaunchKernelGGL(gaussian_filter1d_kernel, dim3(grid_for(T, 256)), dim3(256), 0, h->stream, dx.p, (long long)T, dw.p,
                           radius, dout.p);
    c.download(out, dout);
    return c.finish();
}

extern "C" int rovmpc_kabsch_velocity_transform(rovmpc_handle *h, const double *P, const double *Q, const double *v, int64_t T,
                                                int32_t M, int32_t batch_gates, double *v_out, double *R_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (T < 0 || M < 1 || M > 4096 || (T > 0 && (!P || !Q || !v || !v_out)))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_kabsch_velocity_transform: bad argument");
    if (T == 0) return ROVMPC_OK;
    HelperCall c(h);
    const auto dP = c.upload(P, (size_t)T * M * 3);
    const auto dQ = c.upload(Q, (size_t)T * M * 3);
    const auto dv = c.upload(v, (size_t)T * 3);
    const auto dout = c.buffer<double>((size_t)T * 3);
    const auto dR = c.buffer<double>((size_t)T * 9);
    if (c.ok())
        hipLaunchKernelGGL(kabsch_kernel, dim3(grid_for(T, 128)), dim3(128), 0, h->stream, dP.p, dQ.p, dv.p, (long long)T, M,
                           batch_gates, dout.p, R_out ? dR.p : nullptr);
    c.download(v_out, dout);
    c.download(R_out, dR);
    return c.finish();
}

// ---- (theta, gamma) from cable markers (fit_kernels.h) -----------------------------------------

extern "C" void rovmpc_default_fit_params(rovmpc_fit_params *p) {
    if (!p) return;
    p->struct_size = (int32_t)sizeof(rovmpc_fit_params);
    p->max_iter = 40;
    p->tol = 1e-12;
}

// the checks both entries share, then the kernel's arguments but for the pointers
static int fit_args(rovmpc_handle *h, const char *entry, const void *P0, const void *P1, const void *Y, int64_t B, int32_t M,
                    const rovmpc_fit_params *params, const void *out, FitArgs &a) {
    rovmpc_fit_params p;
    rovmpc_default_fit_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(rovmpc_fit_params))
            FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_fit_params.struct_size %d != %d (ABI mismatch)", params->struct_size, (int)sizeof(rovmpc_fit_params));
        p = *params;
    }
    if (B < 0) FAIL(h, ROVMPC_ERR_INVALID, "%s: B must be >= 0 (got %lld)", entry, (long long)B);
    if (M < 3 || M > ROVMPC_FIT_MAX_MARKERS) FAIL(h, ROVMPC_ERR_INVALID, "%s: M must be in 3..%d (got %d)", entry, ROVMPC_FIT_MAX_MARKERS, M);
    if (!(p.tol >= 0)) FAIL(h, ROVMPC_ERR_INVALID, "%s: tol must be >= 0 (got %g)", entry, p.tol);
    if (p.max_iter < 1 || p.max_iter > 1000) FAIL(h, ROVMPC_ERR_INVALID, "%s: max_iter must be in 1..1000 (got %d)", entry, p.max_iter);
    if (B > 0 && (!P0 || !P1 || !Y || !out)) FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (P0, P1, Y or out)", entry);
    const rovmpc_config &c = h->cfg;
    const bool f64 = c.dtype == ROVMPC_F64;
    memset(&a, 0, sizeof(a));
    a.L = f64 ? c.L : (double)(float)c.L; a.c_lo = f64 ? c.c_lo : (double)(float)c.c_lo; a.c_hi = f64 ? c.c_hi : (double)(float)c.c_hi;
    a.up = c.frame == ROVMPC_ENU ? 1.0 : -1.0;
    a.tol = p.tol; a.B = B; a.M = M; a.max_iter = p.max_iter;
    return ROVMPC_OK;
}

static void launch_fit(rovmpc_handle *h, const FitArgs &a) {
    hipLaunchKernelGGL(fit_theta_gamma_kernel, dim3(grid_for(a.B, FIT_FRAMES)), dim3(FIT_NT), 0, h->stream, a);
}

extern "C" int rovmpc_fit_theta_gamma(rovmpc_handle *h, const double *P0, const double *P1, const double *Y, int64_t B, int32_t M,
                                      const double *guess, const rovmpc_fit_params *params, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    FitArgs a;
    if (int rc = fit_args(h, "rovmpc_fit_theta_gamma", P0, P1, Y, B, M, params, out, a)) return rc;
    if (B == 0) return ROVMPC_OK;
    if (B > (int64_t)1 << 24) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_fit_theta_gamma: more than 2^24 frames in one call (got %lld)", (long long)B);
    HelperCall c(h);
    const auto d0 = c.upload(P0, (size_t)B * 3);
    const auto d1 = c.upload(P1, (size_t)B * 3);
    const auto dY = c.upload(Y, (size_t)B * M * 3);
    const auto dG = guess ? c.upload(guess, (size_t)B * 2) : DevArray<double>{nullptr, 0};
    const auto dO = c.buffer<double>((size_t)B * ROVMPC_FIT_OUT);
    a.P0 = d0.p; a.P1 = d1.p; a.Y = dY.p; a.guess = dG.p; a.out = dO.p;
    if (c.ok()) launch_fit(h, a);
    c.download(out, dO);
    return c.finish();
}

extern "C" int rovmpc_fit_theta_gamma_device(rovmpc_handle *h, const double *d_P0, const double *d_P1, const double *d_Y, int64_t B,
                                             int32_t M, const double *d_guess, const rovmpc_fit_params *params, double *d_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    FitArgs a;
    if (int rc = fit_args(h, "rovmpc_fit_theta_gamma_device", d_P0, d_P1, d_Y, B, M, params, d_out, a)) return rc;
    if (B == 0) return ROVMPC_OK;
    if (B > (int64_t)1 << 24) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_fit_theta_gamma_device: more than 2^24 frames in one call (got %lld)", (long long)B);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    a.P0 = d_P0; a.P1 = d_P1; a.Y = d_Y; a.guess = d_guess; a.out = d_out;
    launch_fit(h, a);
    return launched(h, "marker fit");
}

// ---- the cable length from marker recordings, markers by arc length (calib_kernels.h) ----------

extern "C" void rovmpc_default_calib_params(rovmpc_calib_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(rovmpc_calib_params);
    p->max_iter = 60;
    p->free_length = 1;
    p->L0 = NAN;
    p->L_lo = 0.0; p->L_hi = INFINITY;
    p->tol = 1e-12; p->tol_L = 1e-12;
}

// The handle's working buffers of the calibration: one device block [records | group records | done words | offsets], the
// host copy the offsets are uploaded from and the event behind that upload (the copy is not rewritten before it).
struct CalibWork {
    void *d = nullptr;
    size_t bytes = 0;
    std::vector<int32_t> off_host;
    hipEvent_t ev = nullptr;
};

void calib_free(rovmpc_handle *h) {
    if (!h->calib) return;
    if (h->calib->ev) (void)hipEventDestroy(h->calib->ev);
    if (h->calib->d) (void)hipFree(h->calib->d);
    delete h->calib;
    h->calib = nullptr;
}

// `arc` as the law wants it, into the kernel's argument
static int calib_arc(rovmpc_handle *h, const char *entry, const double *arc, int32_t M, double *dst, int *has_arc) {
    *has_arc = arc != nullptr;
    for (int m = 0; m < ROVMPC_FIT_MAX_MARKERS; ++m) dst[m] = 0.0;
    if (!arc) return ROVMPC_OK;
    for (int m = 0; m < M; ++m) {
        if (!std::isfinite(arc[m]) || (m > 0 && !(arc[m] > arc[m - 1])))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: arc must be finite and strictly increasing (arc[%d] = %g)", entry, m, arc[m]);
        dst[m] = arc[m];
    }
    if (arc[0] != 0.0 || arc[M - 1] != 1.0) FAIL(h, ROVMPC_ERR_INVALID, "%s: arc must run from 0 to 1 (got %g .. %g)", entry, arc[0], arc[M - 1]);
    return ROVMPC_OK;
}

// the checks both entries share, then the kernel's arguments but for the pointers
static int calib_args(rovmpc_handle *h, const char *entry, const void *P0, const void *P1, const void *Y, int64_t F, int32_t M,
                      const int32_t *group_off, int32_t G, const double *arc, const rovmpc_calib_params *params, const void *out_group,
                      const void *out_frame, CalibArgs &a) {
    rovmpc_calib_params p;
    rovmpc_default_calib_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(rovmpc_calib_params))
            FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_calib_params.struct_size %d != %d (ABI mismatch)", params->struct_size, (int)sizeof(rovmpc_calib_params));
        p = *params;
    }
    if (F < 0 || G < 0) FAIL(h, ROVMPC_ERR_INVALID, "%s: F and G must be >= 0 (got %lld, %d)", entry, (long long)F, G);
    if (F > (int64_t)1 << 24) FAIL(h, ROVMPC_ERR_INVALID, "%s: more than 2^24 frames in one call (got %lld)", entry, (long long)F);
    if (M < 3 || M > ROVMPC_FIT_MAX_MARKERS) FAIL(h, ROVMPC_ERR_INVALID, "%s: M must be in 3..%d (got %d)", entry, ROVMPC_FIT_MAX_MARKERS, M);
    if (!(p.tol >= 0) || !(p.tol_L >= 0)) FAIL(h, ROVMPC_ERR_INVALID, "%s: tol and tol_L must be >= 0 (got %g, %g)", entry, p.tol, p.tol_L);
    if (p.max_iter < 1 || p.max_iter > 1000) FAIL(h, ROVMPC_ERR_INVALID, "%s: max_iter must be in 1..1000 (got %d)", entry, p.max_iter);
    const rovmpc_config &c = h->cfg;
    const bool f64 = c.dtype == ROVMPC_F64;
    memset(&a, 0, sizeof(a));
    a.L0 = std::isnan(p.L0) ? (f64 ? c.L : (double)(float)c.L) : p.L0;
    if (!(a.L0 > 0) || !std::isfinite(a.L0)) FAIL(h, ROVMPC_ERR_INVALID, "%s: L0 must be positive and finite (got %g)", entry, p.L0);
    if (!(p.L_lo < p.L_hi)) FAIL(h, ROVMPC_ERR_INVALID, "%s: the box (L_lo, L_hi) is empty (got %g, %g)", entry, p.L_lo, p.L_hi);
    if (p.free_length && !(p.L_lo < a.L0 && a.L0 < p.L_hi))
        FAIL(h, ROVMPC_ERR_INVALID, "%s: L0 = %g lies outside the box (%g, %g)", entry, a.L0, p.L_lo, p.L_hi);
    if (int rc = calib_arc(h, entry, arc, M, a.arc, &a.has_arc)) return rc;
    if (F > 0 && G > 0) {
        if (!P0 || !P1 || !Y || !group_off || !out_group || !out_frame)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (P0, P1, Y, group_off, out_group or out_frame)", entry);
        if (group_off[0] != 0 || (int64_t)group_off[G] != F)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off must run from 0 to F = %lld (got %d .. %d)", entry, (long long)F, group_off[0], group_off[G]);
        for (int g = 0; g < G; ++g)
            if (group_off[g + 1] < group_off[g]) FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off decreases at group %d", entry, g);
    }
    a.L_lo = p.L_lo; a.L_hi = p.L_hi;
    a.c_lo = f64 ? c.c_lo : (double)(float)c.c_lo; a.c_hi = f64 ? c.c_hi : (double)(float)c.c_hi;
    a.up = c.frame == ROVMPC_ENU ? 1.0 : -1.0;
    a.tol = p.tol; a.tol_L = p.tol_L; a.F = F; a.G = G; a.M = M; a.max_iter = p.max_iter; a.free_length = p.free_length != 0;
    return ROVMPC_OK;
}

// The working buffers for F frames in G groups, grown on demand, and the offsets uploaded behind whatever the stream holds.
static int calib_bind(rovmpc_handle *h, const int32_t *group_off, CalibArgs &a) {
    if (!h->calib) h->calib = new CalibWork();
    CalibWork &w = *h->calib;
    const size_t n_rec = (size_t)CF_FIELDS * a.F, n_grp = (size_t)CG_FIELDS * a.G;
    const size_t bytes = (n_rec + n_grp) * sizeof(double) + ((size_t)a.G + (size_t)a.G + 1) * sizeof(int);
    if (!w.ev) HIPCHK(h, hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
    else HIPCHK(h, hipEventSynchronize(w.ev));                              // the upload of the call before has read off_host
    if (bytes > w.bytes) {
        HIPCHK(h, hipStreamSynchronize(h->stream));                         // (growth only: a call before may still use the old block)
        if (w.d) (void)hipFree(w.d);
        w.d = nullptr; w.bytes = 0;
        HIPCHK(h, hipMalloc(&w.d, bytes));
        w.bytes = bytes;
    }
    a.rec = (double *)w.d;
    a.grp = a.rec + n_rec;
    a.done = (int *)(a.grp + n_grp);
    int *d_off = a.done + a.G;
    a.group_off = d_off;
    w.off_host.assign(group_off, group_off + a.G + 1);
    HIPCHK(h, hipMemcpyAsync(d_off, w.off_host.data(), ((size_t)a.G + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(w.ev, h->stream));
    return ROVMPC_OK;
}

static void launch_calib_pair(rovmpc_handle *h, CalibArgs &a, int k) {
    a.launch = k;
    hipLaunchKernelGGL(calib_frames_kernel, dim3(grid_for(a.F, FIT_FRAMES)), dim3(FIT_NT), 0, h->stream, a);
    hipLaunchKernelGGL(calib_reduce_kernel, dim3((unsigned)a.G), dim3(CALIB_RNT), 0, h->stream, a);
}

constexpr int CALIB_BATCH = 8;               // pairs the host entry enqueues between two looks at the done words

extern "C" int rovmpc_calibrate_cable(rovmpc_handle *h, const double *P0, const double *P1, const double *Y, int64_t F, int32_t M,
                                      const int32_t *group_off, int32_t G, const double *guess, const double *arc,
                                      const rovmpc_calib_params *params, double *out_group, double *out_frame) {
    if (!h) return ROVMPC_ERR_INVALID;
    CalibArgs a;
    if (int rc = calib_args(h, "rovmpc_calibrate_cable", P0, P1, Y, F, M, group_off, G, arc, params, out_group, out_frame, a)) return rc;
    if (F == 0 || G == 0) return ROVMPC_OK;
    HelperCall c(h);
    if (!c.ok()) return c.finish();
    if (int rc = calib_bind(h, group_off, a)) return rc;
    const auto d0 = c.upload(P0, (size_t)F * 3);
    const auto d1 = c.upload(P1, (size_t)F * 3);
    const auto dY = c.upload(Y, (size_t)F * M * 3);
    const auto dG = guess ? c.upload(guess, (size_t)F * 2) : DevArray<double>{nullptr, 0};
    const auto dOg = c.buffer<double>((size_t)G * ROVMPC_CALIB_GROUP_OUT);
    const auto dOf = c.buffer<double>((size_t)F * ROVMPC_CALIB_FRAME_OUT);
    a.P0 = d0.p; a.P1 = d1.p; a.Y = dY.p; a.guess = dG.p; a.out_group = dOg.p; a.out_frame = dOf.p;
    std::vector<int> done((size_t)G);
    for (int k = 0; c.ok() && k <= a.max_iter;) {
        for (int i = 0; i < CALIB_BATCH && k <= a.max_iter; ++i, ++k) launch_calib_pair(h, a, k);
        if (k > a.max_iter) break;
        hipError_t e = hipMemcpyAsync(done.data(), a.done, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "reading the done words failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
        bool all = true;
        for (int g = 0; g < G; ++g) all = all && done[g] != 0;
        if (all) break;
    }
    c.download(out_group, dOg);
    c.download(out_frame, dOf);
    return c.finish();
}

extern "C" int rovmpc_calibrate_cable_device(rovmpc_handle *h, const double *d_P0, const double *d_P1, const double *d_Y, int64_t F,
                                             int32_t M, const int32_t *group_off, int32_t G, const double *d_guess, const double *arc,
                                             const rovmpc_calib_params *params, double *d_out_group, double *d_out_frame) {
    if (!h) return ROVMPC_ERR_INVALID;
    CalibArgs a;
    if (int rc = calib_args(h, "rovmpc_calibrate_cable_device", d_P0, d_P1, d_Y, F, M, group_off, G, arc, params, d_out_group, d_out_frame, a))
        return rc;
    if (F == 0 || G == 0) return ROVMPC_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = calib_bind(h, group_off, a)) return rc;
    a.P0 = d_P0; a.P1 = d_P1; a.Y = d_Y; a.guess = d_guess; a.out_group = d_out_group; a.out_frame = d_out_frame;
    for (int k = 0; k <= a.max_iter; ++k) launch_calib_pair(h, a, k);
    return launched(h, "cable calibration");
}

extern "C" int rovmpc_cable_markers(rovmpc_handle *h, const double *P0, const double *P1, const double *theta, const double *gamma,
                                    const double *L, const double *arc, int64_t B, int32_t M, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    const char *entry = "rovmpc_cable_markers";
    if (B < 0 || B > (int64_t)1 << 24) FAIL(h, ROVMPC_ERR_INVALID, "%s: B must be in 0..2^24 (got %lld)", entry, (long long)B);
    if (M < 3 || M > ROVMPC_FIT_MAX_MARKERS) FAIL(h, ROVMPC_ERR_INVALID, "%s: M must be in 3..%d (got %d)", entry, ROVMPC_FIT_MAX_MARKERS, M);
    MarkersArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = calib_arc(h, entry, arc, M, a.arc, &a.has_arc)) return rc;
    if (B > 0 && (!P0 || !P1 || !theta || !gamma || !out)) FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (P0, P1, theta, gamma or out)", entry);
    if (B == 0) return ROVMPC_OK;
    const rovmpc_config &cf = h->cfg;
    const bool f64 = cf.dtype == ROVMPC_F64;
    a.L = f64 ? cf.L : (double)(float)cf.L; a.c_lo = f64 ? cf.c_lo : (double)(float)cf.c_lo; a.c_hi = f64 ? cf.c_hi : (double)(float)cf.c_hi;
    a.up = cf.frame == ROVMPC_ENU ? 1.0 : -1.0;
    a.B = B; a.M = M;
    HelperCall c(h);
    const auto d0 = c.upload(P0, (size_t)B * 3);
    const auto d1 = c.upload(P1, (size_t)B * 3);
    const auto dt = c.upload(theta, (size_t)B);
    const auto dg = c.upload(gamma, (size_t)B);
    const auto dL = L ? c.upload(L, (size_t)B) : DevArray<double>{nullptr, 0};
    const auto dO = c.buffer<double>((size_t)B * M * 3);
    a.P0 = d0.p; a.P1 = d1.p; a.theta = dt.p; a.gamma = dg.p; a.Lb = dL.p; a.out = dO.p;
    if (c.ok()) hipLaunchKernelGGL(cable_markers_kernel, dim3(grid_for(B * M, 256)), dim3(256), 0, h->stream, a);
    c.download(out, dO);
    return c.finish();
}

// ---- (theta, gamma) along marker recordings (track_kernels.h) ----------------------------------

extern "C" void rovmpc_default_track_params(rovmpc_track_params *p) {
    if (!p) return;
    rovmpc_fit_params f;
    rovmpc_default_fit_params(&f);
    memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(rovmpc_track_params);
    p->n_starts = 5;
    p->max_iter = f.max_iter;
    p->tol = f.tol;
    p->rms_max = HUGE_VAL;
    const double th[5] = {0.0, 0.3, -0.3, 0.6, -0.6};
    for (int k = 0; k < 5; ++k) p->starts[k][0] = th[k];
}

// the checks both entries share, then the kernel's arguments but for the pointers
static int track_args(rovmpc_handle *h, const char *entry, const void *P0, const void *P1, const void *Y, int64_t B, int64_t T, int32_t M,
                      const rovmpc_track_params *params, const void *out, TrackArgs &a) {
    rovmpc_track_params p;
    rovmpc_default_track_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(rovmpc_track_params))
            FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_track_params.struct_size %d != %d (ABI mismatch)", params->struct_size, (int)sizeof(rovmpc_track_params));
        p = *params;
    }
    if (T < 0) FAIL(h, ROVMPC_ERR_INVALID, "%s: T must be >= 0 (got %lld)", entry, (long long)T);
    if (p.n_starts < 1 || p.n_starts > ROVMPC_TRACK_MAX_STARTS)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: n_starts must be in 1..%d (got %d)", entry, ROVMPC_TRACK_MAX_STARTS, p.n_starts);
    for (int k = 0; k < p.n_starts; ++k)
        if (!std::isfinite(p.starts[k][0]) || !std::isfinite(p.starts[k][1]))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: start %d is not finite (%g, %g)", entry, k, p.starts[k][0], p.starts[k][1]);
    if (!(p.rms_max > 0)) FAIL(h, ROVMPC_ERR_INVALID, "%s: rms_max must be > 0 (got %g)", entry, p.rms_max);
    rovmpc_fit_params fp;
    rovmpc_default_fit_params(&fp);
    fp.tol = p.tol; fp.max_iter = p.max_iter;
    FitArgs f;                               // B, M, tol, max_iter and the pointers: the fit's own checks; L, c_lo, c_hi, up as it holds them
    const bool empty = B == 0 || T == 0;
    if (int rc = fit_args(h, entry, empty ? nullptr : P0, empty ? nullptr : P1, empty ? nullptr : Y, empty ? 0 : B, M, &fp, empty ? nullptr : out, f))
        return rc;
    if (B < 0) FAIL(h, ROVMPC_ERR_INVALID, "%s: B must be >= 0 (got %lld)", entry, (long long)B);
    if (!empty && (B > ((int64_t)1 << 24) || T > ((int64_t)1 << 24) || B * T > ((int64_t)1 << 24)))
        FAIL(h, ROVMPC_ERR_INVALID, "%s: more than 2^24 frames in one call (got %lld x %lld)", entry, (long long)B, (long long)T);
    memset(&a, 0, sizeof(a));
    a.L = f.L; a.c_lo = f.c_lo; a.c_hi = f.c_hi; a.up = f.up;
    a.tol = p.tol; a.rms_max = p.rms_max; a.B = B; a.T = T; a.M = M; a.max_iter = p.max_iter; a.n_starts = p.n_starts;
    memcpy(a.starts, p.starts, sizeof(a.starts));
    return ROVMPC_OK;
}

// T frames as launches of at most track_chunk; the stream orders them, and each reads the carry the one before left in `out`
static void launch_track(rovmpc_handle *h, TrackArgs &a) {
    for (long long t0 = 0; t0 < a.T; t0 += h->track_chunk) {
        a.t0 = t0; a.t1 = std::min<long long>(a.T, t0 + h->track_chunk);
        hipLaunchKernelGGL(track_markers_kernel, dim3(grid_for(a.B, FIT_FRAMES)), dim3(FIT_NT), 0, h->stream, a);
    }
}

extern "C" int rovmpc_track_markers(rovmpc_handle *h, const double *P0, const double *P1, const double *Y, int64_t B, int64_t T, int32_t M,
                                    double *carry, const rovmpc_track_params *params, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    TrackArgs a;
    if (int rc = track_args(h, "rovmpc_track_markers", P0, P1, Y, B, T, M, params, out, a)) return rc;
    if (B == 0 || T == 0) return ROVMPC_OK;
    HelperCall c(h);
    const size_t n = (size_t)B * T;
    const auto d0 = c.upload(P0, n * 3);
    const auto d1 = c.upload(P1, n * 3);
    const auto dY = c.upload(Y, n * M * 3);
    const auto dC = carry ? c.upload((const double *)carry, (size_t)B * 2) : DevArray<double>{nullptr, 0};
    const auto dO = c.buffer<double>(n * ROVMPC_TRACK_OUT);
    a.P0 = d0.p; a.P1 = d1.p; a.Y = dY.p; a.carry = dC.p; a.out = dO.p;
    if (c.ok()) launch_track(h, a);
    c.download(out, dO);
    if (carry) c.download(carry, dC);
    return c.finish();
}

extern "C" int rovmpc_track_markers_device(rovmpc_handle *h, const double *d_P0, const double *d_P1, const double *d_Y, int64_t B,
                                           int64_t T, int32_t M, double *d_carry, const rovmpc_track_params *params, double *d_out,
                                           double *d_exo) {
    if (!h) return ROVMPC_ERR_INVALID;
    TrackArgs a;
    if (int rc = track_args(h, "rovmpc_track_markers_device", d_P0, d_P1, d_Y, B, T, M, params, d_out, a)) return rc;
    if (B == 0 || T == 0) return ROVMPC_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    a.P0 = d_P0; a.P1 = d_P1; a.Y = d_Y; a.carry = d_carry; a.out = d_out; a.exo = d_exo;
    launch_track(h, a);
    return launched(h, "marker track");
}

// ---- equation rows scored on recordings (score_kernels.h) --------------------------------------

// The checks of the scoring and the refit entries, in the order the scoring entry has always made them: the sizes of the call,
// (its integrator,) the rows, the lengths.  The non-null pointers are the entry's own to check first.
static int check_row_call(rovmpc_handle *h, const char *entry, int32_t R, int32_t F, int64_t T, int64_t B) {
    if (R < 1 || B < 1 || T < 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: R, B and T must be >= 1 (got %d, %lld, %lld)", entry, R, (long long)B, (long long)T);
    if ((int64_t)R * B > ((int64_t)1 << 24)) FAIL(h, ROVMPC_ERR_INVALID, "%s: more than 2^24 (row, recording) pairs in one call (got %d x %lld)", entry, R, (long long)B);
    if (F < 1 || F > ROVMPC_MAX_FEATURES) FAIL(h, ROVMPC_ERR_INVALID, "%s: F must be in 1..%d (got %d)", entry, ROVMPC_MAX_FEATURES, F);
    return ROVMPC_OK;
}

static int check_programs(rovmpc_handle *h, const char *entry, const int32_t *code, const int32_t *code_off, const double *consts,
                          const int32_t *const_off, int32_t R, int32_t F) {
    if (code_off[0] != 0 || const_off[0] != 0) FAIL(h, ROVMPC_ERR_INVALID, "%s: code_off[0] and const_off[0] must be 0", entry);
    for (int r = 0; r < R; ++r)
        if (code_off[r + 1] < code_off[r] || const_off[r + 1] < const_off[r] || code_off[r + 1] - code_off[r] > ROVMPC_MAX_CODE ||
            const_off[r + 1] - const_off[r] > ROVMPC_MAX_CODE)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: offsets of row %d are not monotone (or the row is longer than %d)", entry, r, ROVMPC_MAX_CODE);
    if (const_off[R] > 0 && !consts) FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (consts)", entry);
    for (int r = 0; r < R; ++r)
        if (const char *why = validate_code(code + code_off[r], code_off[r + 1] - code_off[r], F, const_off[r + 1] - const_off[r]))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: row %d: %s", entry, r, why);
    return ROVMPC_OK;
}

static int check_lengths(rovmpc_handle *h, const char *entry, const int64_t *len, int64_t T, int64_t B) {
    if (len)
        for (int64_t b = 0; b < B; ++b)
            if (len[b] < 1 || len[b] > T) FAIL(h, ROVMPC_ERR_INVALID, "%s: len[%lld] must be in 1..%lld (got %lld)", entry, (long long)b, (long long)T, (long long)len[b]);
    return ROVMPC_OK;
}

// the checked programs and lengths packed for one copy: [consts][len][code][code_off][const_off]
static void pack_programs(const int32_t *code, const int32_t *code_off, const double *consts, const int32_t *const_off, int32_t R,
                          int32_t F, const int64_t *len, int64_t T, int64_t B, std::vector<unsigned char> &blob, ScoreArgs &a) {
    const size_t nk = (size_t)const_off[R], nl = len ? (size_t)B : 0, nc = (size_t)code_off[R], no = (size_t)R + 1;
    const size_t o_len = (nk ? nk : 1) * sizeof(double), o_code = o_len + nl * sizeof(int64_t), o_coff = o_code + nc * sizeof(int32_t),
                 o_koff = o_coff + no * sizeof(int32_t);
    blob.assign(o_koff + no * sizeof(int32_t), 0);
    if (nk) memcpy(blob.data(), consts, nk * sizeof(double));
    if (nl) memcpy(blob.data() + o_len, len, nl * sizeof(int64_t));
    memcpy(blob.data() + o_code, code, nc * sizeof(int32_t));
    memcpy(blob.data() + o_coff, code_off, no * sizeof(int32_t));
    memcpy(blob.data() + o_koff, const_off, no * sizeof(int32_t));
    memset(&a, 0, sizeof(a));
    a.T = T; a.B = B; a.F = F;
    // (offsets into the packed copy until score_bind puts the device address under them)
    a.consts = (const double *)0; a.len = len ? (const long long *)o_len : nullptr; a.code = (const int32_t *)o_code;
    a.code_off = (const int32_t *)o_coff; a.const_off = (const int32_t *)o_koff;
}

// what both scoring entries check, then the packed copy
static int score_args(rovmpc_handle *h, const char *entry, const int32_t *code, const int32_t *code_off, const double *consts,
                      const int32_t *const_off, int32_t R, const void *X, int32_t F, const void *time, const int64_t *len, int64_t T,
                      int64_t B, const void *truth, int32_t integrator, const void *scores, std::vector<unsigned char> &blob, ScoreArgs &a) {
    if (!code || !code_off || !const_off || !X || !time || !truth || !scores)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (code, code_off, const_off, X, time, truth or scores)", entry);
    if (int rc = check_row_call(h, entry, R, F, T, B)) return rc;
    if (integrator < ROVMPC_RK4 || integrator > ROVMPC_TRAPEZOID) FAIL(h, ROVMPC_ERR_INVALID, "%s: unknown integrator %d", entry, integrator);
    if (int rc = check_programs(h, entry, code, code_off, consts, const_off, R, F)) return rc;
    if (int rc = check_lengths(h, entry, len, T, B)) return rc;
    pack_programs(code, code_off, consts, const_off, R, F, len, T, B, blob, a);
    a.integrator = integrator;
    return ROVMPC_OK;
}

static void score_bind(ScoreArgs &a, const unsigned char *d_blob, bool has_len) {
    const unsigned char *base = d_blob;
    a.len = has_len ? (const long long *)(base + (size_t)a.len) : nullptr;
    a.code = (const int32_t *)(base + (size_t)a.code);
    a.code_off = (const int32_t *)(base + (size_t)a.code_off);
    a.const_off = (const int32_t *)(base + (size_t)a.const_off);
    a.consts = (const double *)base;
}

// A device entry's packed host arrays into the handle's buffer, on h->stream (h->d_score_prog is the copy afterwards).
static int stage_programs(rovmpc_handle *h, std::vector<unsigned char> &blob) {
    if (blob.size() > h->score_prog_bytes) {                  // (hipFree waits for the work that still reads the old copy)
        if (h->d_score_prog) HIPCHK(h, hipFree(h->d_score_prog));
        h->d_score_prog = nullptr; h->score_prog_bytes = 0;
        HIPCHK(h, hipMalloc(&h->d_score_prog, blob.size()));
        h->score_prog_bytes = blob.size();
    }
    // The source of the copy is kept in the handle until the copy has run: the caller's arrays may go when the call returns.
    // Only a second call waits, and only for the copy of the call before (the stream orders the new copy behind that launch).
    if (h->score_prog_ev) HIPCHK(h, hipEventSynchronize(h->score_prog_ev));
    else HIPCHK(h, hipEventCreateWithFlags(&h->score_prog_ev, hipEventDisableTiming));
    h->score_prog_host.swap(blob);
    HIPCHK(h, hipMemcpyAsync(h->d_score_prog, h->score_prog_host.data(), h->score_prog_host.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->score_prog_ev, h->stream));
    return ROVMPC_OK;
}

static void launch_score(rovmpc_handle *h, int32_t R, const ScoreArgs &a) {
    hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)((int64_t)R * a.B)), dim3(SCORE_NT), score_lds_bytes(a.F, a.integrator), h->stream, a);
}

extern "C" int rovmpc_score_rows(rovmpc_handle *h, const int32_t *code, const int32_t *code_off, const double *consts,
                                 const int32_t *const_off, int32_t R, const double *X, int32_t F, const double *time, const int64_t *len,
                                 int64_t T, int64_t B, const double *truth, const double *target, const double *y0, int32_t integrator,
                                 double *scores, double *est, double *pred) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    ScoreArgs a;
    if (int rc = score_args(h, "rovmpc_score_rows", code, code_off, consts, const_off, R, X, F, time, len, T, B, truth, integrator, scores, blob, a))
        return rc;
    HelperCall c(h);
    const size_t n = (size_t)B * T, rows = (size_t)R * B;
    const auto dP = c.upload((const unsigned char *)blob.data(), blob.size());
    const auto dX = c.upload(X, n * F);
    const auto dT = c.upload(time, n);
    const auto dY = c.upload(truth, n);
    const auto dG = target ? c.upload(target, n) : DevArray<double>{nullptr, 0};
    const auto d0 = y0 ? c.upload(y0, (size_t)B) : DevArray<double>{nullptr, 0};
    const auto dS = c.buffer<double>(rows * ROVMPC_SCORE_COLS);
    const auto dE = est ? c.buffer<double>(rows * T) : DevArray<double>{nullptr, 0};
    const auto dR = pred ? c.buffer<double>(rows * T) : DevArray<double>{nullptr, 0};
    score_bind(a, dP.p, len != nullptr);
    a.X = dX.p; a.time = dT.p; a.truth = dY.p; a.target = dG.p; a.y0 = d0.p; a.scores = dS.p; a.est = dE.p; a.pred = dR.p;
    if (c.ok()) launch_score(h, R, a);
    c.download(scores, dS);
    if (est) c.download(est, dE);
    if (pred) c.download(pred, dR);
    return c.finish();
}

extern "C" int rovmpc_score_rows_device(rovmpc_handle *h, const int32_t *code, const int32_t *code_off, const double *consts,
                                        const int32_t *const_off, int32_t R, const double *d_X, int32_t F, const double *d_time,
                                        const int64_t *len, int64_t T, int64_t B, const double *d_truth, const double *d_target,
                                        const double *d_y0, int32_t integrator, double *d_scores, double *d_est, double *d_pred) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    ScoreArgs a;
    if (int rc = score_args(h, "rovmpc_score_rows_device", code, code_off, consts, const_off, R, d_X, F, d_time, len, T, B, d_truth, integrator,
                            d_scores, blob, a))
        return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = stage_programs(h, blob)) return rc;
    score_bind(a, (const unsigned char *)h->d_score_prog, len != nullptr);
    a.X = d_X; a.time = d_time; a.truth = d_truth; a.target = d_target; a.y0 = d_y0; a.scores = d_scores; a.est = d_est; a.pred = d_pred;
    launch_score(h, R, a);
    return launched(h, "row scoring");
}

// ---- constants of equation rows refitted on recordings (refit_kernels.h) -----------------------

extern "C" void rovmpc_default_refit_params(rovmpc_refit_params *p) {
    if (!p) return;
    p->struct_size = (int32_t)sizeof(rovmpc_refit_params);
    p->max_iter = 50;
    p->gtol = 1e-10;
    p->xtol = 1e-12;
}

namespace {
// a checked call: the kernel's arguments with offsets into the packed copy where refit_bind puts device addresses
struct RefitPlan {
    ScoreArgs s;                                  // the programs and lengths, packed as for rovmpc_score_rows
    size_t o_group, o_fidx, o_nfree;              // behind them: group offsets, free indices per row, their counts
    bool has_len;
    RefitArgs a;
};
}  // namespace

// the checks both entries share; then everything the kernel reads from host arrays packed for one copy
static int refit_args(rovmpc_handle *h, const char *entry, const int32_t *code, const int32_t *code_off, const double *consts,
                      const int32_t *const_off, const uint8_t *free_mask, int32_t R, const void *X, int32_t F, const int64_t *len,
                      int64_t T, int64_t B, const void *target, const int32_t *group_off, int32_t G, const rovmpc_refit_params *params,
                      const void *consts_out, const void *out, std::vector<unsigned char> &blob, RefitPlan &plan) {
    if (!code || !code_off || !const_off || !X || !target || !consts_out || !out)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (code, code_off, const_off, X, target, consts_out or out)", entry);
    if (int rc = check_row_call(h, entry, R, F, T, B)) return rc;
    if (int rc = check_programs(h, entry, code, code_off, consts, const_off, R, F)) return rc;
    if (int rc = check_lengths(h, entry, len, T, B)) return rc;
    if (G < 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: G must be >= 1 (got %d)", entry, G);
    if ((int64_t)R * G > ((int64_t)1 << 24)) FAIL(h, ROVMPC_ERR_INVALID, "%s: more than 2^24 (row, group) pairs in one call (got %d x %d)", entry, R, G);
    if (!group_off && G != 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off is NULL, which pools all recordings: G must be 1 (got %d)", entry, G);
    if (group_off) {
        if (group_off[0] != 0 || (int64_t)group_off[G] != B)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off must run from 0 to B = %lld (got %d .. %d)", entry, (long long)B, group_off[0], group_off[G]);
        for (int g = 0; g < G; ++g)
            if (group_off[g + 1] <= group_off[g]) FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off must increase (group %d is empty or runs backwards)", entry, g);
    }
    rovmpc_refit_params p;
    rovmpc_default_refit_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(rovmpc_refit_params))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: rovmpc_refit_params.struct_size %d != %d (ABI mismatch)", entry, params->struct_size, (int)sizeof(rovmpc_refit_params));
        p = *params;
    }
    if (p.max_iter < 1 || p.max_iter > 1000) FAIL(h, ROVMPC_ERR_INVALID, "%s: max_iter must be in 1..1000 (got %d)", entry, p.max_iter);
    if (!(p.gtol >= 0.0) || !(p.xtol >= 0.0)) FAIL(h, ROVMPC_ERR_INVALID, "%s: gtol and xtol must be >= 0 (got %g, %g)", entry, p.gtol, p.xtol);
    // per row: the free constants in pool order, and the stack simulation once more with one bit per slot -- whether a free
    // constant reaches the value -- for the exponent of a POW; its deepest point sizes the kernel's operand stacks
    std::vector<int32_t> fidx((size_t)R * ROVMPC_REFIT_MAX_PARAMS, 0), nfree((size_t)R, 0);
    int depth = 1;
    for (int r = 0; r < R; ++r) {
        const int k0 = const_off[r], nk = const_off[r + 1] - k0;
        int P = 0;
        for (int k = 0; k < nk; ++k) {
            if (free_mask && !free_mask[k0 + k]) continue;
            if (P < ROVMPC_REFIT_MAX_PARAMS) fidx[(size_t)r * ROVMPC_REFIT_MAX_PARAMS + P] = k;
            ++P;
        }
        if (P > ROVMPC_REFIT_MAX_PARAMS)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: row %d: %d free constants (at most %d)", entry, r, P, ROVMPC_REFIT_MAX_PARAMS);
        nfree[r] = P;
        unsigned char st[ROVMPC_MAX_STACK];
        int sp = 0;
        for (int pc = code_off[r]; pc < code_off[r + 1]; ++pc) {
            const int op = code[pc] & 0xff, arg = code[pc] >> 8;
            if (op == ROVMPC_OP_PUSH_C) st[sp++] = !free_mask || free_mask[k0 + arg];
            else if (op == ROVMPC_OP_PUSH_F) st[sp++] = 0;
            else if ((op >= ROVMPC_OP_ADD && op <= ROVMPC_OP_DIV) || op == ROVMPC_OP_POW) {
                if (op == ROVMPC_OP_POW && st[sp - 1]) FAIL(h, ROVMPC_ERR_INVALID, "%s: row %d: free constant in a POW exponent", entry, r);
                st[sp - 2] = st[sp - 2] | st[sp - 1];
                --sp;
            }
            if (sp > depth) depth = sp;
        }
    }
    pack_programs(code, code_off, consts, const_off, R, F, len, T, B, blob, plan.s);
    const size_t o_group = (blob.size() + 7) & ~(size_t)7, o_fidx = o_group + ((size_t)G + 1) * sizeof(int64_t),
                 o_nfree = o_fidx + fidx.size() * sizeof(int32_t);
    blob.resize(o_nfree + nfree.size() * sizeof(int32_t), 0);
    int64_t *go = (int64_t *)(blob.data() + o_group);
    for (int g = 0; g <= G; ++g) go[g] = group_off ? (int64_t)group_off[g] : (g ? B : 0);
    memcpy(blob.data() + o_fidx, fidx.data(), fidx.size() * sizeof(int32_t));
    memcpy(blob.data() + o_nfree, nfree.data(), nfree.size() * sizeof(int32_t));
    plan.o_group = o_group; plan.o_fidx = o_fidx; plan.o_nfree = o_nfree; plan.has_len = len != nullptr;
    RefitArgs &a = plan.a;
    memset(&a, 0, sizeof(a));
    a.T = T; a.B = B; a.G = G; a.nk = const_off[R]; a.F = F; a.depth = depth; a.max_iter = p.max_iter; a.gtol = p.gtol; a.xtol = p.xtol;
    return ROVMPC_OK;
}

static void refit_bind(RefitPlan &plan, const unsigned char *d_blob) {
    score_bind(plan.s, d_blob, plan.has_len);
    RefitArgs &a = plan.a;
    a.code = plan.s.code; a.code_off = plan.s.code_off; a.consts = plan.s.consts; a.const_off = plan.s.const_off; a.len = plan.s.len;
    a.group_off = (const long long *)(d_blob + plan.o_group);
    a.free_idx = (const int32_t *)(d_blob + plan.o_fidx);
    a.n_free = (const int32_t *)(d_blob + plan.o_nfree);
}

static void launch_refit(rovmpc_handle *h, int32_t R, const RefitArgs &a) {
    hipLaunchKernelGGL(refit_rows_kernel, dim3((unsigned)((int64_t)R * a.G)), dim3(SCORE_NT), refit_lds_bytes(a.depth), h->stream, a);
}

extern "C" int rovmpc_refit_rows(rovmpc_handle *h, const int32_t *code, const int32_t *code_off, const double *consts,
                                 const int32_t *const_off, const uint8_t *free_mask, int32_t R, const double *X, int32_t F,
                                 const int64_t *len, int64_t T, int64_t B, const double *target, const int32_t *group_off, int32_t G,
                                 const rovmpc_refit_params *params, double *consts_out, double *out) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    RefitPlan plan;
    if (int rc = refit_args(h, "rovmpc_refit_rows", code, code_off, consts, const_off, free_mask, R, X, F, len, T, B, target, group_off, G,
                            params, consts_out, out, blob, plan))
        return rc;
    HelperCall c(h);
    const size_t n = (size_t)B * T;
    const auto dP = c.upload((const unsigned char *)blob.data(), blob.size());
    const auto dX = c.upload(X, n * F);
    const auto dG = c.upload(target, n);
    const auto dK = c.buffer<double>((size_t)G * (size_t)plan.a.nk);
    const auto dO = c.buffer<double>((size_t)R * G * ROVMPC_REFIT_OUT);
    refit_bind(plan, dP.p);
    plan.a.X = dX.p; plan.a.target = dG.p; plan.a.consts_out = dK.p; plan.a.out = dO.p;
    if (c.ok()) launch_refit(h, R, plan.a);
    if (plan.a.nk > 0) c.download(consts_out, dK);
    c.download(out, dO);
    return c.finish();
}

extern "C" int rovmpc_refit_rows_device(rovmpc_handle *h, const int32_t *code, const int32_t *code_off, const double *consts,
                                        const int32_t *const_off, const uint8_t *free_mask, int32_t R, const double *d_X, int32_t F,
                                        const int64_t *len, int64_t T, int64_t B, const double *d_target, const int32_t *group_off,
                                        int32_t G, const rovmpc_refit_params *params, double *d_consts_out, double *d_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    RefitPlan plan;
    if (int rc = refit_args(h, "rovmpc_refit_rows_device", code, code_off, consts, const_off, free_mask, R, d_X, F, len, T, B, d_target,
                            group_off, G, params, d_consts_out, d_out, blob, plan))
        return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = stage_programs(h, blob)) return rc;
    refit_bind(plan, (const unsigned char *)h->d_score_prog);
    plan.a.X = d_X; plan.a.target = d_target; plan.a.consts_out = d_consts_out; plan.a.out = d_out;
    launch_refit(h, R, plan.a);
    return launched(h, "row refit");
}

// ---- equation rows discovered by sparse regression over a term library (discover_kernels.h) ----

extern "C" void rovmpc_default_discover_params(rovmpc_discover_params *p) {
    if (!p) return;
    p->struct_size = (int32_t)sizeof(rovmpc_discover_params);
    p->max_terms = ROVMPC_DISCOVER_MAX_SIZE;
    p->dep_tol = 1e-10;
    p->min_gain = 1e-12;
}

namespace {
// a checked call: the kernels' arguments with offsets into the packed copy where discover_bind puts device addresses
struct DiscoverPlan {
    ScoreArgs s;                                  // the programs and lengths, packed as for rovmpc_score_rows
    size_t o_crec, o_crow, o_gchunk, o_gn;        // behind them: the chunk table and the groups' chunk ranges and row counts
    size_t n_chunks, E;
    bool has_len;
    DiscoverArgs a;
};
}  // namespace

// the checks both entries share; then everything the kernels read from host arrays packed for one copy
static int discover_args(rovmpc_handle *h, const char *entry, const int32_t *code, const int32_t *code_off, const double *consts,
                         const int32_t *const_off, int32_t M, const void *X, int32_t F, const int64_t *len, int64_t T, int64_t B,
                         const void *target, const int32_t *group_off, int32_t G, const rovmpc_discover_params *params,
                         const void *picks, const void *coef, const void *loss, const void *info, std::vector<unsigned char> &blob,
                         DiscoverPlan &plan) {
    if (!code || !code_off || !const_off || !X || !target || !picks || !coef || !loss || !info)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (code, code_off, const_off, X, target, picks, coef, loss or info)", entry);
    if (M < 1 || M > ROVMPC_DISCOVER_MAX_TERMS) FAIL(h, ROVMPC_ERR_INVALID, "%s: M must be in 1..%d (got %d)", entry, ROVMPC_DISCOVER_MAX_TERMS, M);
    if (int rc = check_row_call(h, entry, M, F, T, B)) return rc;
    if (int rc = check_programs(h, entry, code, code_off, consts, const_off, M, F)) return rc;
    if (int rc = check_lengths(h, entry, len, T, B)) return rc;
    if (G < 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: G must be >= 1 (got %d)", entry, G);
    if (!group_off && G != 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off is NULL, which pools all recordings: G must be 1 (got %d)", entry, G);
    if (group_off) {
        if (group_off[0] != 0 || (int64_t)group_off[G] != B)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off must run from 0 to B = %lld (got %d .. %d)", entry, (long long)B, group_off[0], group_off[G]);
        for (int g = 0; g < G; ++g)
            if (group_off[g + 1] <= group_off[g]) FAIL(h, ROVMPC_ERR_INVALID, "%s: group_off must increase (group %d is empty or runs backwards)", entry, g);
    }
    rovmpc_discover_params p;
    rovmpc_default_discover_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(rovmpc_discover_params))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: rovmpc_discover_params.struct_size %d != %d (ABI mismatch)", entry, params->struct_size, (int)sizeof(rovmpc_discover_params));
        p = *params;
    }
    if (p.max_terms < 1 || p.max_terms > ROVMPC_DISCOVER_MAX_SIZE)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: max_terms must be in 1..%d (got %d)", entry, ROVMPC_DISCOVER_MAX_SIZE, p.max_terms);
    if (!(p.dep_tol >= 0.0) || !(p.min_gain >= 0.0)) FAIL(h, ROVMPC_ERR_INVALID, "%s: dep_tol and min_gain must be >= 0 (got %g, %g)", entry, p.dep_tol, p.min_gain);
    // the chunk table: recording after recording, chunk after chunk, so a group's chunks are one range in the law's order
    const int64_t per_full = (T + ROVMPC_DISCOVER_CHUNK - 1) / ROVMPC_DISCOVER_CHUNK;
    if (per_full > ((int64_t)1 << 24) || per_full * B > ((int64_t)1 << 24))
        FAIL(h, ROVMPC_ERR_INVALID, "%s: more than 2^24 chunks of %d rows in one call (got %lld x %lld rows)", entry, ROVMPC_DISCOVER_CHUNK, (long long)B, (long long)T);
    std::vector<int64_t> crec, crow, gchunk((size_t)G + 1, 0), gn((size_t)G, 0);
    for (int g = 0; g < G; ++g) {
        const int64_t b0 = group_off ? group_off[g] : 0, b1 = group_off ? group_off[g + 1] : B;
        for (int64_t b = b0; b < b1; ++b) {
            const int64_t n = len ? len[b] : T;
            for (int64_t r0 = 0; r0 < n; r0 += ROVMPC_DISCOVER_CHUNK) { crec.push_back(b); crow.push_back(r0); }
            gn[g] += n;
        }
        gchunk[g + 1] = (int64_t)crec.size();
    }
    pack_programs(code, code_off, consts, const_off, M, F, len, T, B, blob, plan.s);
    const size_t nc = crec.size();
    plan.o_crec = (blob.size() + 7) & ~(size_t)7;
    plan.o_crow = plan.o_crec + nc * sizeof(int64_t);
    plan.o_gchunk = plan.o_crow + nc * sizeof(int64_t);
    plan.o_gn = plan.o_gchunk + gchunk.size() * sizeof(int64_t);
    blob.resize(plan.o_gn + gn.size() * sizeof(int64_t), 0);
    memcpy(blob.data() + plan.o_crec, crec.data(), nc * sizeof(int64_t));
    memcpy(blob.data() + plan.o_crow, crow.data(), nc * sizeof(int64_t));
    memcpy(blob.data() + plan.o_gchunk, gchunk.data(), gchunk.size() * sizeof(int64_t));
    memcpy(blob.data() + plan.o_gn, gn.data(), gn.size() * sizeof(int64_t));
    plan.n_chunks = nc; plan.E = (size_t)(M + 1) * (M + 2) / 2; plan.has_len = len != nullptr;
    DiscoverArgs &a = plan.a;
    memset(&a, 0, sizeof(a));
    a.T = T; a.F = F; a.M = M; a.S = p.max_terms; a.dep_tol = p.dep_tol; a.min_gain = p.min_gain;
    return ROVMPC_OK;
}

static void discover_bind(DiscoverPlan &plan, const unsigned char *d_blob) {
    score_bind(plan.s, d_blob, plan.has_len);
    DiscoverArgs &a = plan.a;
    a.code = plan.s.code; a.code_off = plan.s.code_off; a.consts = plan.s.consts; a.const_off = plan.s.const_off; a.len = plan.s.len;
    a.chunk_rec = (const long long *)(d_blob + plan.o_crec);
    a.chunk_row = (const long long *)(d_blob + plan.o_crow);
    a.group_chunk = (const long long *)(d_blob + plan.o_gchunk);
    a.group_n = (const long long *)(d_blob + plan.o_gn);
}

// the handle's buffer of chunk partials, at least n doubles (hipFree waits for the work that still reads the old one)
static int discover_partials(rovmpc_handle *h, size_t n) {
    if (n > h->discover_partial_n) {
        if (h->d_discover_partial) HIPCHK(h, hipFree(h->d_discover_partial));
        h->d_discover_partial = nullptr; h->discover_partial_n = 0;
        HIPCHK(h, hipMalloc(&h->d_discover_partial, n * sizeof(double)));
        h->discover_partial_n = n;
    }
    return ROVMPC_OK;
}

static void launch_discover(rovmpc_handle *h, int32_t G, const DiscoverPlan &plan) {
    hipLaunchKernelGGL(discover_gram_kernel, dim3((unsigned)plan.n_chunks), dim3(DISC_NT), discover_gram_lds_bytes(plan.a.M), h->stream, plan.a);
    hipLaunchKernelGGL(discover_select_kernel, dim3((unsigned)G), dim3(DISC_WAVE), 0, h->stream, plan.a);
}

extern "C" int rovmpc_discover_rows(rovmpc_handle *h, const int32_t *code, const int32_t *code_off, const double *consts,
                                    const int32_t *const_off, int32_t M, const double *X, int32_t F, const int64_t *len, int64_t T,
                                    int64_t B, const double *target, const int32_t *group_off, int32_t G,
                                    const rovmpc_discover_params *params, int32_t *picks, double *coef, double *loss, int64_t *info,
                                    double *gram) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    DiscoverPlan plan;
    if (int rc = discover_args(h, "rovmpc_discover_rows", code, code_off, consts, const_off, M, X, F, len, T, B, target, group_off, G, params,
                               picks, coef, loss, info, blob, plan))
        return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = discover_partials(h, plan.n_chunks * plan.E)) return rc;
    HelperCall c(h);
    const size_t n = (size_t)B * T, S = (size_t)plan.a.S;
    const auto dP = c.upload((const unsigned char *)blob.data(), blob.size());
    const auto dX = c.upload(X, n * F);
    const auto dT = c.upload(target, n);
    const auto dK = c.buffer<int32_t>((size_t)G * S);
    const auto dC = c.buffer<double>((size_t)G * S * S);
    const auto dL = c.buffer<double>((size_t)G * (S + 1));
    const auto dI = c.buffer<long long>((size_t)G * 3);
    const auto dG = gram ? c.buffer<double>((size_t)G * plan.E) : DevArray<double>{nullptr, 0};
    discover_bind(plan, dP.p);
    plan.a.X = dX.p; plan.a.target = dT.p; plan.a.partial = h->d_discover_partial;
    plan.a.picks = dK.p; plan.a.coef = dC.p; plan.a.loss = dL.p; plan.a.info = dI.p; plan.a.gram = dG.p;
    if (c.ok()) launch_discover(h, G, plan);
    c.download(picks, dK);
    c.download(coef, dC);
    c.download(loss, dL);
    c.download((long long *)info, dI);
    if (gram) c.download(gram, dG);
    return c.finish();
}

extern "C" int rovmpc_discover_rows_device(rovmpc_handle *h, const int32_t *code, const int32_t *code_off, const double *consts,
                                           const int32_t *const_off, int32_t M, const double *d_X, int32_t F, const int64_t *len,
                                           int64_t T, int64_t B, const double *d_target, const int32_t *group_off, int32_t G,
                                           const rovmpc_discover_params *params, int32_t *d_picks, double *d_coef, double *d_loss,
                                           int64_t *d_info, double *d_gram) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    DiscoverPlan plan;
    if (int rc = discover_args(h, "rovmpc_discover_rows_device", code, code_off, consts, const_off, M, d_X, F, len, T, B, d_target, group_off,
                               G, params, d_picks, d_coef, d_loss, d_info, blob, plan))
        return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = discover_partials(h, plan.n_chunks * plan.E)) return rc;
    if (int rc = stage_programs(h, blob)) return rc;
    discover_bind(plan, (const unsigned char *)h->d_score_prog);
    plan.a.X = d_X; plan.a.target = d_target; plan.a.partial = h->d_discover_partial;
    plan.a.picks = d_picks; plan.a.coef = d_coef; plan.a.loss = d_loss; plan.a.info = (long long *)d_info; plan.a.gram = d_gram;
    launch_discover(h, G, plan);
    return launched(h, "row discovery");
}

// ---- (theta, gamma) row pairs scored by closed-loop N-step-ahead skill (horizon_kernels.h) -----

extern "C" void rovmpc_default_horizon_params(rovmpc_horizon_params *p) {
    if (!p) return;
    p->struct_size = (int32_t)sizeof(rovmpc_horizon_params);
    p->integrator = ROVMPC_RK4;
    p->prev_mode = ROVMPC_PREV_INTERP;
    p->H = 20;
    p->stride = 1;
    p->slot_theta = 14; p->slot_gamma = 15; p->slot_theta_prev = 16; p->slot_gamma_prev = 17;
    p->slot_cos_theta = -1; p->slot_sin_gamma = -1;
}

// one front of a pair call: its offsets and its rows, named by the front in the message
static int check_front(rovmpc_handle *h, const char *entry, const char *front, const int32_t *code, const int32_t *code_off,
                       const double *consts, const int32_t *const_off, int32_t R, int32_t F) {
    if (code_off[0] != 0 || const_off[0] != 0) FAIL(h, ROVMPC_ERR_INVALID, "%s: %s front: code_off[0] and const_off[0] must be 0", entry, front);
    for (int r = 0; r < R; ++r)
        if (code_off[r + 1] < code_off[r] || const_off[r + 1] < const_off[r] || code_off[r + 1] - code_off[r] > ROVMPC_MAX_CODE ||
            const_off[r + 1] - const_off[r] > ROVMPC_MAX_CODE)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: offsets of %s row %d are not monotone (or the row is longer than %d)", entry, front, r, ROVMPC_MAX_CODE);
    if (const_off[R] > 0 && !consts) FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (consts of the %s front)", entry, front);
    for (int r = 0; r < R; ++r)
        if (const char *why = validate_code(code + code_off[r], code_off[r + 1] - code_off[r], F, const_off[r + 1] - const_off[r]))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: %s row %d: %s", entry, front, r, why);
    return ROVMPC_OK;
}

namespace {
// a checked call: the kernel's arguments with offsets into the packed copy where horizon_bind puts device addresses
struct HorizonPlan {
    HorizonArgs a;
    size_t o_g, o_pairs;                          // behind the theta front: the gamma front, the pairs
    bool has_len;
};
}  // namespace

// the checks both entries share; then everything the kernel reads from host arrays packed for one copy
static int horizon_args(rovmpc_handle *h, const char *entry, const int32_t *code_t, const int32_t *code_off_t, const double *consts_t,
                        const int32_t *const_off_t, int32_t Rt, const int32_t *code_g, const int32_t *code_off_g, const double *consts_g,
                        const int32_t *const_off_g, int32_t Rg, const int32_t *pairs, int32_t Q, const void *X, int32_t F,
                        const double *mean, const double *scale, const void *time, const int64_t *len, int64_t T, int64_t B,
                        const void *theta, const void *gamma, const rovmpc_horizon_params *params, const void *skill,
                        std::vector<unsigned char> &blob, HorizonPlan &plan) {
    if (!code_t || !code_off_t || !const_off_t || !code_g || !code_off_g || !const_off_g || !pairs || !X || !mean || !scale || !time ||
        !theta || !gamma || !skill)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (a front's code, code_off or const_off, pairs, X, mean, scale, time, theta, gamma or skill)", entry);
    if (Q < 1 || B < 1 || T < 1 || Rt < 1 || Rg < 1)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: Q, B, T, Rt and Rg must be >= 1 (got %d, %lld, %lld, %d, %d)", entry, Q, (long long)B, (long long)T, Rt, Rg);
    if ((int64_t)Q * B > ((int64_t)1 << 24)) FAIL(h, ROVMPC_ERR_INVALID, "%s: more than 2^24 (pair, recording) problems in one call (got %d x %lld)", entry, Q, (long long)B);
    if (F < 1 || F > ROVMPC_MAX_FEATURES) FAIL(h, ROVMPC_ERR_INVALID, "%s: F must be in 1..%d (got %d)", entry, ROVMPC_MAX_FEATURES, F);
    rovmpc_horizon_params p;
    rovmpc_default_horizon_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(rovmpc_horizon_params))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: rovmpc_horizon_params.struct_size %d != %d (ABI mismatch)", entry, params->struct_size, (int)sizeof(rovmpc_horizon_params));
        p = *params;
    }
    if (p.H < 1 || p.stride < 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: H and stride must be >= 1 (got %d, %d)", entry, p.H, p.stride);
    if (p.integrator != ROVMPC_RK4 && p.integrator != ROVMPC_EULER)
        FAIL(h, ROVMPC_ERR_INVALID, "%s: integrator must be ROVMPC_RK4 or ROVMPC_EULER (got %d; the second-order maps are not provided)", entry, p.integrator);
    if (p.prev_mode != ROVMPC_PREV_INTERP && p.prev_mode != ROVMPC_PREV_HOLD) FAIL(h, ROVMPC_ERR_INVALID, "%s: unknown prev_mode %d", entry, p.prev_mode);
    for (int q = 0; q < Q; ++q)
        if (pairs[2 * q] < 0 || pairs[2 * q] >= Rt || pairs[2 * q + 1] < 0 || pairs[2 * q + 1] >= Rg)
            FAIL(h, ROVMPC_ERR_INVALID, "%s: pair %d = (%d, %d) is outside the fronts (%d theta rows, %d gamma rows)", entry, q, pairs[2 * q], pairs[2 * q + 1], Rt, Rg);
    static const char *const names[HZ_SLOTS] = {"slot_theta", "slot_gamma", "slot_theta_prev", "slot_gamma_prev", "slot_cos_theta", "slot_sin_gamma"};
    const int32_t slots[HZ_SLOTS] = {p.slot_theta, p.slot_gamma, p.slot_theta_prev, p.slot_gamma_prev, p.slot_cos_theta, p.slot_sin_gamma};
    if (p.slot_theta == -1 || p.slot_gamma == -1) FAIL(h, ROVMPC_ERR_INVALID, "%s: slot_theta and slot_gamma are required (got %d, %d)", entry, p.slot_theta, p.slot_gamma);
    for (int k = 0; k < HZ_SLOTS; ++k) {
        if (slots[k] == -1) continue;
        if (slots[k] < 0 || slots[k] >= F) FAIL(h, ROVMPC_ERR_INVALID, "%s: %s = %d is outside 0..%d", entry, names[k], slots[k], F - 1);
        for (int m = 0; m < k; ++m)
            if (slots[m] == slots[k]) FAIL(h, ROVMPC_ERR_INVALID, "%s: %s and %s both name slot %d", entry, names[m], names[k], slots[k]);
        if (scale[slots[k]] == 0.0 || !std::isfinite(scale[slots[k]]) || !std::isfinite(mean[slots[k]]))
            FAIL(h, ROVMPC_ERR_INVALID, "%s: mean and scale of %s (slot %d) must be finite, the scale not 0 (got %g, %g)", entry, names[k], slots[k],
                 mean[slots[k]], scale[slots[k]]);
    }
    if (int rc = check_front(h, entry, "theta", code_t, code_off_t, consts_t, const_off_t, Rt, F)) return rc;
    if (int rc = check_front(h, entry, "gamma", code_g, code_off_g, consts_g, const_off_g, Rg, F)) return rc;
    if (int rc = check_lengths(h, entry, len, T, B)) return rc;
    HorizonArgs &a = plan.a;
    memset(&a, 0, sizeof(a));
    std::vector<unsigned char> blob_g;
    pack_programs(code_t, code_off_t, consts_t, const_off_t, Rt, F, len, T, B, blob, a.t);
    pack_programs(code_g, code_off_g, consts_g, const_off_g, Rg, F, nullptr, T, B, blob_g, a.g);
    plan.o_g = (blob.size() + 7) & ~(size_t)7;
    plan.o_pairs = plan.o_g + ((blob_g.size() + 7) & ~(size_t)7);
    blob.resize(plan.o_pairs + (size_t)Q * 2 * sizeof(int32_t), 0);
    memcpy(blob.data() + plan.o_g, blob_g.data(), blob_g.size());
    memcpy(blob.data() + plan.o_pairs, pairs, (size_t)Q * 2 * sizeof(int32_t));
    plan.has_len = len != nullptr;
    a.H = p.H; a.stride = p.stride; a.integrator = p.integrator; a.prev_mode = p.prev_mode;
    a.W = horizon_windows(T, p.H, p.stride);
    for (int k = 0; k < HZ_SLOTS; ++k) {
        a.slot[k] = slots[k];
        a.mean[k] = slots[k] >= 0 ? mean[slots[k]] : 0.0;
        a.scale[k] = slots[k] >= 0 ? scale[slots[k]] : 1.0;
    }
    return ROVMPC_OK;
}

static void horizon_bind(HorizonPlan &plan, const unsigned char *d_blob) {
    score_bind(plan.a.t, d_blob, plan.has_len);
    score_bind(plan.a.g, d_blob + plan.o_g, false);
    plan.a.pairs = (const int32_t *)(d_blob + plan.o_pairs);
}

static void launch_horizon(rovmpc_handle *h, int32_t Q, const HorizonArgs &a) {
    hipLaunchKernelGGL(score_pairs_kernel, dim3((unsigned)((int64_t)Q * a.t.B)), dim3(HORIZON_NT), horizon_lds_bytes(a.t.F), h->stream, a);
}

extern "C" int rovmpc_score_pairs(rovmpc_handle *h, const int32_t *code_t, const int32_t *code_off_t, const double *consts_t,
                                  const int32_t *const_off_t, int32_t Rt, const int32_t *code_g, const int32_t *code_off_g,
                                  const double *consts_g, const int32_t *const_off_g, int32_t Rg, const int32_t *pairs, int32_t Q,
                                  const double *X, int32_t F, const double *mean, const double *scale, const double *time,
                                  const int64_t *len, int64_t T, int64_t B, const double *theta, const double *gamma,
                                  const rovmpc_horizon_params *params, double *skill, double *pred) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    HorizonPlan plan;
    if (int rc = horizon_args(h, "rovmpc_score_pairs", code_t, code_off_t, consts_t, const_off_t, Rt, code_g, code_off_g, consts_g, const_off_g,
                              Rg, pairs, Q, X, F, mean, scale, time, len, T, B, theta, gamma, params, skill, blob, plan))
        return rc;
    HelperCall c(h);
    HorizonArgs &a = plan.a;
    const size_t n = (size_t)B * T, problems = (size_t)Q * B, n_pred = problems * (size_t)a.W * a.H * 2;
    const auto dP = c.upload((const unsigned char *)blob.data(), blob.size());
    const auto dX = c.upload(X, n * F);
    const auto dT = c.upload(time, n);
    const auto dA = c.upload(theta, n);
    const auto dG = c.upload(gamma, n);
    const auto dS = c.buffer<double>(problems * a.H * ROVMPC_HORIZON_COLS);
    const auto dR = pred && n_pred ? c.buffer<double>(n_pred) : DevArray<double>{nullptr, 0};
    horizon_bind(plan, dP.p);
    a.t.X = dX.p; a.t.time = dT.p; a.theta = dA.p; a.gamma = dG.p; a.skill = dS.p; a.pred = dR.p;
    if (c.ok()) launch_horizon(h, Q, a);
    c.download(skill, dS);
    if (dR.p) c.download(pred, dR);
    return c.finish();
}

extern "C" int rovmpc_score_pairs_device(rovmpc_handle *h, const int32_t *code_t, const int32_t *code_off_t, const double *consts_t,
                                         const int32_t *const_off_t, int32_t Rt, const int32_t *code_g, const int32_t *code_off_g,
                                         const double *consts_g, const int32_t *const_off_g, int32_t Rg, const int32_t *pairs, int32_t Q,
                                         const double *d_X, int32_t F, const double *mean, const double *scale, const double *d_time,
                                         const int64_t *len, int64_t T, int64_t B, const double *d_theta, const double *d_gamma,
                                         const rovmpc_horizon_params *params, double *d_skill, double *d_pred) {
    if (!h) return ROVMPC_ERR_INVALID;
    std::vector<unsigned char> blob;
    HorizonPlan plan;
    if (int rc = horizon_args(h, "rovmpc_score_pairs_device", code_t, code_off_t, consts_t, const_off_t, Rt, code_g, code_off_g, consts_g,
                              const_off_g, Rg, pairs, Q, d_X, F, mean, scale, d_time, len, T, B, d_theta, d_gamma, params, d_skill, blob, plan))
        return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = stage_programs(h, blob)) return rc;
    HorizonArgs &a = plan.a;
    horizon_bind(plan, (const unsigned char *)h->d_score_prog);
    a.t.X = d_X; a.t.time = d_time; a.theta = d_theta; a.gamma = d_gamma; a.skill = d_skill; a.pred = a.W > 0 ? d_pred : nullptr;
    launch_horizon(h, Q, a);
    return launched(h, "pair scoring");
}
