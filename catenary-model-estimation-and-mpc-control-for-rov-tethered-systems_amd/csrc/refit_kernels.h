// refit_kernels.h -- rovmpc_refit_rows: the constants of R expressions refitted to the derivative target on G groups of
// recordings by Levenberg-Marquardt (fp64, gfx950).  The law is in include/rovmpc.h; one workgroup per (row, group), no
// atomics, nothing between workgroups.  The value of a row is interp_eval's, its sums are score_kernels.h's; new here are the
// tangents of a row with respect to its free constants and the solver around them.
#pragma once
#include "score_kernels.h"

namespace rovmpc {

constexpr int REFIT_MP = ROVMPC_REFIT_MAX_PARAMS;
// the sums of one Jacobian pass, row j of the lower triangle followed by its gradient entry: A_j0 .. A_jj, g_j
constexpr int REFIT_CHUNK = 9;                                  // sums reduced per round of the tree (the stack's LDS holds them)
constexpr int REFIT_NSUM = 45;                                  // MP (MP + 3) / 2 = 44, rounded up to whole chunks
RV_DEV constexpr int refit_row0(int j) { return j * (j + 3) / 2; }
static_assert(refit_row0(REFIT_MP) <= REFIT_NSUM && REFIT_NSUM % REFIT_CHUNK == 0, "the chunks cover the sums");

struct RefitArgs {
    const int32_t *code, *code_off;              // [code_off[R]], [R + 1]
    const double *consts;                        // [const_off[R]]: the starts
    const int32_t *const_off;                    // [R + 1]
    const long long *len;                        // [B] or null
    const long long *group_off;                  // [G + 1]
    const int32_t *free_idx, *n_free;            // [R][REFIT_MP] constant indices within the row's slice, [R]
    const double *X, *target;                    // [B][T][F], [B][T]
    double *consts_out, *out;                    // [G][const_off[R]], [R][G][ROVMPC_REFIT_OUT]
    long long T, B, G, nk;                       // nk = const_off[R]: the constants of one group in consts_out
    int F, depth, max_iter;                      // depth: the deepest operand stack of the call's rows
    double gtol, xtol;
};

// stack region in doubles per lane: value and tangent stacks, and never less than one round of the tree
__host__ __device__ inline int refit_region(int depth) { return 2 * depth > REFIT_CHUNK ? 2 * depth : REFIT_CHUNK; }
inline size_t refit_lds_bytes(int depth) { return (size_t)(refit_region(depth) + REFIT_MP) * SCORE_NT * sizeof(double); }

RV_DEV double refit_sign(double a) { return a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : 0.0); }

// square-and-multiply as interp_eval's POWI
RV_DEV double refit_powi(double b, int e) {
    int ae = e < 0 ? -e : e;
    double r = 1.0;
    while (ae) { if (ae & 1) r *= b; b *= b; ae >>= 1; }
    return e < 0 ? 1.0 / r : r;
}

// interp_eval on dual numbers: the value by the same operations, beside it the tangent along constant `kfree` of the row
// (the table of include/rovmpc.h).  Both operand stacks live in LDS ([depth][lane]), the tops in registers.
RV_DEV void refit_dual_eval(const int32_t *__restrict__ code, int n, const double *consts, int kfree, const double *feat,
                            double *vs, double *ts, int ss, double &value, double &tangent) {
#pragma clang fp contract(off)
    double v = 0.0, d = 0.0;
    int sp = 0;
    for (int pc = 0; pc < n; ++pc) {
        const int ins = code[pc];
        const int op = ins & 0xff, arg = ins >> 8;
        double a = 0.0, da = 0.0;
        if ((op >= ROVMPC_OP_ADD && op <= ROVMPC_OP_DIV) || op == ROVMPC_OP_POW) { a = vs[(sp - 2) * ss]; da = ts[(sp - 2) * ss]; --sp; }
        switch (op) {
        case ROVMPC_OP_PUSH_C:
            if (sp > 0) { vs[(sp - 1) * ss] = v; ts[(sp - 1) * ss] = d; }
            v = consts[arg]; d = arg == kfree ? 1.0 : 0.0; ++sp; break;
        case ROVMPC_OP_PUSH_F:
            if (sp > 0) { vs[(sp - 1) * ss] = v; ts[(sp - 1) * ss] = d; }
            v = feat[arg]; d = 0.0; ++sp; break;
        case ROVMPC_OP_ADD: v = a + v; d = da + d; break;
        case ROVMPC_OP_SUB: v = a - v; d = da - d; break;
        case ROVMPC_OP_MUL: d = da * v + a * d; v = a * v; break;
        case ROVMPC_OP_DIV: { const double q = m_divx(a, v); d = (da - q * d) / v; v = q; break; }
        case ROVMPC_OP_POW: { const double w = m_pow(a, v); d = da * v * m_pow(a, v - 1.0); v = w; break; }
        case ROVMPC_OP_NEG: v = -v; d = -d; break;
        case ROVMPC_OP_SIN: d = d * m_cos(v); v = m_sin(v); break;
        case ROVMPC_OP_COS: d = -(d * m_sin(v)); v = m_cos(v); break;
        case ROVMPC_OP_TANH: { const double t = m_tanh(v); d = d * (1.0 - t * t); v = t; break; }
        case ROVMPC_OP_ABS: d = d * refit_sign(v); v = m_abs(v); break;
        case ROVMPC_OP_SQUARE: d = (2.0 * v) * d; v = v * v; break;
        case ROVMPC_OP_EXP: { const double e = m_exp(v); d = d * e; v = e; break; }
        case ROVMPC_OP_LOG: d = d / v; v = m_log(v); break;
        case ROVMPC_OP_SQRT: { const double s = m_sqrt(v); d = d / (2.0 * s); v = s; break; }
        case ROVMPC_OP_POWI: {
            const int e = arg >= (1 << 23) ? arg - (1 << 24) : arg;     // signed 24-bit
            d = e == 0 ? 0.0 : ((double)e * refit_powi(v, e - 1)) * d;
            v = refit_powi(v, e); break;
        }
        case ROVMPC_OP_SAFE_LOG: { const double s = m_abs(v) + 1e-5; d = d * refit_sign(v) / s; v = m_log(s); break; }
        case ROVMPC_OP_SAFE_SQRT: { const double s = m_sqrt(m_abs(v)); d = d * refit_sign(v) / (2.0 * s); v = s; break; }
        default: v = m_nan<double>(); d = v; break;
        }
    }
    value = v; tangent = d;
}

// one (row, group): what the passes over the group's recordings read
struct RefitProblem {
    const int32_t *code;
    int ncode, F;
    long long T, b0, b1;
    const long long *len;
    const double *X, *target;
};

// F = sum (g - p)^2 over the group's counted rows in the law's order, p by interp_eval itself.  All lanes call and return F.
RV_DEV double refit_sum_F(const RefitProblem &q, const double *consts, double *lds, int lane) {
#pragma clang fp contract(off)
    constexpr int NT = SCORE_NT;
    double acc = 0.0;
    for (long long b = q.b0; b < q.b1; ++b) {
        const long long n = q.len ? q.len[b] : q.T;
        const double *X = q.X + (size_t)b * q.T * q.F, *g = q.target + (size_t)b * q.T;
        for (long long t0 = 0; t0 < n; t0 += NT) {
            const long long i0 = t0 + lane, i = i0 < n ? i0 : n - 1;    // rows past n repeat the last one: uniform control flow
            const double p = interp_eval<double>(q.code, q.ncode, consts, X + i * q.F, 1, lds + lane, NT);
            if (i0 < n) { const double dp = g[i0] - p; acc = acc + dp * dp; }
        }
    }
    lds[lane] = acc;
    score_tree_sum(lds, lane);
    const double F = lds[0];
    __syncthreads();
    return F;
}

// A = J^T J (lower triangle) and g = J^T r at `consts` into sums[] (layout: refit_row0), one tangent direction per pass of the
// interpreter.  All lanes call; returns whether an entry of J was not finite.
RV_DEV bool refit_sum_J(const RefitProblem &q, const double *consts, int P, const int *idx, int depth, double *lds, double *sJ,
                        double *sums, int lane) {
#pragma clang fp contract(off)
    constexpr int NT = SCORE_NT, MP = REFIT_MP;
    double acc[REFIT_NSUM];
#pragma unroll
    for (int k = 0; k < REFIT_NSUM; ++k) acc[k] = 0.0;
    bool bad = false;
    double *const vs = lds + lane, *const ts = lds + (size_t)depth * NT + lane, *const J = sJ + lane;
    for (long long b = q.b0; b < q.b1; ++b) {
        const long long n = q.len ? q.len[b] : q.T;
        const double *X = q.X + (size_t)b * q.T * q.F, *g = q.target + (size_t)b * q.T;
        for (long long t0 = 0; t0 < n; t0 += NT) {
            const long long i0 = t0 + lane, i = i0 < n ? i0 : n - 1;
            double p = 0.0;
            for (int j = 0; j < P; ++j) {
                double dp;
                refit_dual_eval(q.code, q.ncode, consts, idx[j], X + i * q.F, vs, ts, NT, p, dp);
                J[j * NT] = dp;
            }
            if (i0 < n) {
                const double r = p - g[i0];
                double Jr[MP];
#pragma unroll
                for (int j = 0; j < MP; ++j) Jr[j] = j < P ? J[j * NT] : 0.0;
#pragma unroll
                for (int j = 0; j < MP; ++j) {
                    if (j < P) {
                        bad = bad || !m_finite(Jr[j]);
#pragma unroll
                        for (int k = 0; k <= j; ++k) acc[refit_row0(j) + k] = acc[refit_row0(j) + k] + Jr[j] * Jr[k];
                        acc[refit_row0(j) + j + 1] = acc[refit_row0(j) + j + 1] + Jr[j] * r;
                    }
                }
            }
        }
    }
    // the law's tree, REFIT_CHUNK sums per round (the operand stacks' LDS is free now; every lane writes its own column)
    const int nsum = refit_row0(P);
#pragma unroll
    for (int c = 0; c < REFIT_NSUM / REFIT_CHUNK; ++c) {
        if (c * REFIT_CHUNK < nsum) {
#pragma unroll
            for (int k = 0; k < REFIT_CHUNK; ++k) lds[k * NT + lane] = acc[c * REFIT_CHUNK + k];
            for (int s = NT / 2; s > 0; s >>= 1) {
                __syncthreads();
                if (lane < s)
                    for (int k = 0; k < REFIT_CHUNK; ++k) lds[k * NT + lane] = lds[k * NT + lane] + lds[k * NT + lane + s];
            }
            __syncthreads();
            if (lane < REFIT_CHUNK) sums[c * REFIT_CHUNK + lane] = lds[lane * NT];
            __syncthreads();
        }
    }
    return __syncthreads_or(bad) != 0;
}

// MINPACK's orthogonality measure max_j |g_j| / sqrt(A_jj F) over the j with A_jj > 0; 0 when F = 0 (one lane)
RV_DEV double refit_orth(const double *sums, int P, double F) {
#pragma clang fp contract(off)
    if (F == 0.0) return 0.0;
    double o = 0.0;
    for (int j = 0; j < P; ++j) {
        const double ajj = sums[refit_row0(j) + j], gj = sums[refit_row0(j) + j + 1];
        if (ajj > 0.0) { const double v = ::fabs(gj) / ::sqrt(ajj * F); o = (v > o || v != v) ? v : o; }
    }
    return o;
}

// (A + mu diag A) delta = -g by Cholesky (one lane); false when a pivot is <= 0 or not a number
RV_DEV bool refit_solve(const double *sums, int P, double mu, double *L, double *delta) {
#pragma clang fp contract(off)
    constexpr int MP = REFIT_MP;
    for (int j = 0; j < P; ++j) {
        for (int k = 0; k <= j; ++k) {
            double s = sums[refit_row0(j) + k];
            if (k == j) s = s + mu * s;
            for (int m = 0; m < k; ++m) s = s - L[j * MP + m] * L[k * MP + m];
            if (k == j) {
                if (!(s > 0.0)) return false;
                L[j * MP + j] = ::sqrt(s);
            } else {
                L[j * MP + k] = s / L[k * MP + k];
            }
        }
    }
    for (int j = 0; j < P; ++j) {                                       // L y = -g
        double s = -sums[refit_row0(j) + j + 1];
        for (int m = 0; m < j; ++m) s = s - L[j * MP + m] * delta[m];
        delta[j] = s / L[j * MP + j];
    }
    for (int j = P - 1; j >= 0; --j) {                                  // L^T delta = y
        double s = delta[j];
        for (int m = j + 1; m < P; ++m) s = s - L[m * MP + j] * delta[m];
        delta[j] = s / L[j * MP + j];
    }
    return true;
}

__global__ void __launch_bounds__(SCORE_NT)
refit_rows_kernel(const RefitArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    constexpr int NT = SCORE_NT, MP = REFIT_MP;
    const int lane = threadIdx.x;
    double *const lds = reinterpret_cast<double *>(smem_raw);          // value stack, tangent stack: [depth][lane] each
    double *const sJ = lds + (size_t)refit_region(a.depth) * NT;        // J_i[0 .. P) of the lane's row: [MP][lane]
    __shared__ double sC[ROVMPC_MAX_CODE], sT[ROVMPC_MAX_CODE];        // the iterate and the trial: the row's whole slice
    __shared__ double sCur[REFIT_NSUM], sSum[REFIT_NSUM];              // A and g at the iterate and at the trial
    __shared__ double sL[MP * MP], sD[MP], sCtl[3];                    // Cholesky factor, step, (orth, solved, small)
    __shared__ int sIdx[MP];
    const long long r = blockIdx.x / a.G, grp = blockIdx.x % a.G;
    const int k0 = a.const_off[r], nk = a.const_off[r + 1] - k0, P = a.n_free[r];
    RefitProblem q;
    q.code = a.code + a.code_off[r]; q.ncode = a.code_off[r + 1] - a.code_off[r]; q.F = a.F; q.T = a.T;
    q.b0 = a.group_off[grp]; q.b1 = a.group_off[grp + 1]; q.len = a.len; q.X = a.X; q.target = a.target;
    for (int k = lane; k < nk; k += NT) { const double c = a.consts[k0 + k]; sC[k] = c; sT[k] = c; }
    if (lane < MP) sIdx[lane] = lane < P ? a.free_idx[r * MP + lane] : 0;
    long long ntot = 0;
    for (long long b = q.b0; b < q.b1; ++b) ntot += a.len ? a.len[b] : a.T;
    const double dn = (double)ntot, nan = m_nan<double>();
    __syncthreads();

    double F = 0.0, F0 = 0.0, mu = ROVMPC_REFIT_MU0;
    int it = 0, status = ROVMPC_REFIT_MAX_ITER;
    bool first = true, small = false;
    for (;;) {
        // the trial (the start, the first time): F, and A and g only where F lets the trial be taken
        const double Ft = refit_sum_F(q, sT, lds, lane);
        bool take = m_finite(Ft) && (first || Ft <= F);
        if (take && P > 0) take = !refit_sum_J(q, sT, P, sIdx, a.depth, lds, sJ, sSum, lane);
        if (first) {
            F0 = Ft; F = Ft;
            if (P == 0) { status = ROVMPC_REFIT_NO_PARAMS; break; }
            if (!take) { status = ROVMPC_REFIT_NONFINITE; break; }
        }
        if (take) {
            for (int k = lane; k < nk; k += NT) sC[k] = sT[k];
            if (lane < REFIT_NSUM) sCur[lane] = sSum[lane];
            F = Ft;
            if (!first) mu = ::fmax(mu / 10.0, ROVMPC_REFIT_MU_MIN);
        } else {
            mu = mu * 10.0;
        }
        __syncthreads();
        if (!first && small) { status = ROVMPC_REFIT_CONVERGED; break; }
        first = false;
        // before a trial
        if (lane == 0) sCtl[0] = refit_orth(sCur, P, F);
        __syncthreads();
        if (F == 0.0 || sCtl[0] <= a.gtol) { status = ROVMPC_REFIT_CONVERGED; break; }
        bool solved = false;
        for (;;) {
            if (mu > ROVMPC_REFIT_MU_MAX) { status = ROVMPC_REFIT_STALLED; break; }
            if (it == a.max_iter) { status = ROVMPC_REFIT_MAX_ITER; break; }
            ++it;
            if (lane == 0) {
                const bool ok = refit_solve(sCur, P, mu, sL, sD);
                bool sm = ok;
                for (int j = 0; ok && j < P; ++j) sm = sm && ::fabs(sD[j]) <= a.xtol * (::fabs(sC[sIdx[j]]) + a.xtol);
                sCtl[1] = ok ? 1.0 : 0.0; sCtl[2] = sm ? 1.0 : 0.0;
            }
            __syncthreads();
            solved = sCtl[1] != 0.0;
            small = sCtl[2] != 0.0;
            if (solved) break;
            mu = mu * 10.0;                                             // a pivot <= 0 or not a number: a rejected trial
            __syncthreads();
        }
        if (!solved) break;
        for (int k = lane; k < nk; k += NT) sT[k] = sC[k];
        __syncthreads();
        if (lane < P) sT[sIdx[lane]] = sC[sIdx[lane]] + sD[lane];
        __syncthreads();
    }

    __syncthreads();
    double *cout = a.consts_out + (size_t)grp * a.nk + k0;
    for (int k = lane; k < nk; k += NT) cout[k] = sC[k];
    if (lane == 0) {
        double *o = a.out + ((size_t)r * a.G + grp) * ROVMPC_REFIT_OUT;
        const bool nonfinite = status == ROVMPC_REFIT_NONFINITE;
        o[0] = F0 / dn;
        o[1] = nonfinite ? nan : F / dn;
        o[2] = nonfinite ? nan : (P > 0 ? refit_orth(sCur, P, F) : 0.0);
        o[3] = (double)it;
        o[4] = (double)status;
        o[5] = (double)P;
    }
}

}  // namespace rovmpc
