// proposal_kernels.h -- the shaped proposal of MPPI and CEM on gfx950 (rovmpc_set_noise_correlation, rovmpc_mppi_set_bounds):
// time-correlated sampling noise along the horizon and a box on the candidates.  The law is stated in include/rovmpc.h
// above rovmpc_set_noise_correlation.  With beta all zero and no MPPI box these kernels are not launched: the white
// samplers (mppi_sample_kernel, cem_sample_kernel and their batched forms) run as before.
#pragma once
#include "cem_kernels.h"

namespace rovmpc {

// Both controllers draw U[0] = (T) clamp(m), U[k][n][c] = (T) clamp(fma(s[n][c], eps[k][n][c], m[n][c])) for k >= 1 with
//   eps[k][0][c] = z[k][0][c],  eps[k][n][c] = fma(beta[c], eps[k][n-1][c], root[c] * z[k][n][c]),  root = sqrt((1 - beta)(1 + beta)),
// z_e the white samplers' stream (one Philox block = four consecutive elements e).  MPPI: m = nu, s = std[c], the handle's
// box; CEM: m = mu, s = sigma (null: std[c]), its parameters' box.
//
// The recurrence runs along n, so one thread must own a (k, c) pair, while the stream comes four consecutive elements at a
// time: a workgroup takes a tile of `rows` whole candidate rows (a multiple of 4, so every tile starts on a Philox block for
// any N) and exchanges through LDS:
//   1. thread j draws Philox block j of the tile, as the white samplers do, and stores its four z;
//   2. thread t walks (row t / 3, channel t % 3) over n and leaves eps in place of z;
//   3. every thread forms U in element order (coalesced stores).
// A row of the tile has `stride` doubles in LDS, stride = 3 N padded up to 3 mod 32: in phase 2 lane t of a half-wave then
// touches double 3 (t / 3) + t % 3 + 3 n = t + 3 n mod 32, one bank pair each -- no conflict in the 32-lane groups of
// ds_read_b64 nor in the 16-lane groups of ds_write_b64.  Phases 1 and 3 go through rows in element order, where the
// padding only shifts whole rows.  The host picks rows so that a tile has about one Philox block per thread (3 N rows <= 1024
// elements; 4 rows where a row alone is longer) -- proposal_tile() in rovmpc.hip.
constexpr int PROPOSAL_NT = 256;
constexpr int PROPOSAL_CHUNK = 8;           // nodes of phase 2 whose LDS loads are issued together

struct ProposalLaw {
    unsigned long long counter;
    double beta[3], root[3], std[3], lo[3], hi[3];
    long long K;
    int N, rows, stride;                // candidates per tile (multiple of 4), doubles per tile row in LDS (>= 3 N)
    const double *mean;                 // [N][3] (batched: [B][N][3])
    const double *sigma;                // [N][3] / [B][N][3], or null: std[c] on every node
};

// v[c] of a per-channel triple in the kernel arguments by selects: a run-time index would move the arguments to scratch
RV_DEV double proposal_pick(const double (&v)[3], int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }

// the draw of one problem; the batched sampler runs the same body per problem, so the bits are the same
template <typename T>
RV_DEV void proposal_sample_body(unsigned long long seed, const ProposalLaw &a, const double *mean, const double *sigma,
                                 T *__restrict__ U) {
    extern __shared__ __align__(16) unsigned char proposal_smem[];
    double *sE = reinterpret_cast<double *>(proposal_smem);                 // [rows][stride]
    const int tid = threadIdx.x, row3 = 3 * a.N, S = a.stride;
    const long long k0 = (long long)blockIdx.x * a.rows;
    const int rows = a.K - k0 < a.rows ? (int)(a.K - k0) : a.rows;          // the last tile holds fewer
    const int nel = rows * row3;                                            // <= 4096
    const long long e0 = k0 * row3;                                         // a multiple of 4

    // (1) the tile's Philox blocks; the last one may run past the tile's (and the tensor's) end
    for (int jl = tid; 4 * jl < nel; jl += PROPOSAL_NT) {
        double z[4];
        philox_normal4(seed, a.counter, e0 / 4 + jl, z);
        int r = 4 * jl / row3, col = 4 * jl - r * row3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (4 * jl + i < nel) sE[r * S + col] = z[i];
            if (++col == row3) { col = 0; ++r; }
        }
    }
    __syncthreads();

    // (2) z -> eps in place, one (row, channel) per thread along n
    for (int t = tid; t < 3 * rows; t += PROPOSAL_NT) {
        const int c = t % 3;
        double *p = sE + (t / 3) * S + c;
        const double beta = proposal_pick(a.beta, c), root = proposal_pick(a.root, c);
        double eps = p[0];
        for (int n0 = 1; n0 < a.N; n0 += PROPOSAL_CHUNK) {          // one LDS round trip per chunk, not per node
            double z[PROPOSAL_CHUNK];
#pragma unroll
            for (int i = 0; i < PROPOSAL_CHUNK; ++i) z[i] = n0 + i < a.N ? p[3 * (n0 + i)] : 0.0;
#pragma unroll
            for (int i = 0; i < PROPOSAL_CHUNK; ++i) {
                if (n0 + i >= a.N) break;
                eps = ::fma(beta, eps, root * z[i]);
                p[3 * (n0 + i)] = eps;
            }
        }
    }
    __syncthreads();

    // (3) U in element order; (r, col) of element l advance with l by PROPOSAL_NT per pass.  Four passes at a time, their
    //     loads of the plan issued before any is used (a tile of about 1024 elements is one such round)
    const int dr = PROPOSAL_NT / row3, dc = PROPOSAL_NT - dr * row3;
    int r = tid / row3, col = tid - r * row3;
    for (int l0 = tid; l0 < nel; l0 += 4 * PROPOSAL_NT) {
        int rr[4], cc[4];
        double m[4], s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rr[i] = r; cc[i] = col;
            const bool in = l0 + i * PROPOSAL_NT < nel;
            m[i] = in ? mean[col] : 0.0;
            s[i] = in && sigma ? sigma[col] : 0.0;
            r += dr; col += dc;
            if (col >= row3) { col -= row3; ++r; }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = l0 + i * PROPOSAL_NT;
            if (l >= nel) break;
            const int c = cc[i] % 3;
            const double sd = sigma ? s[i] : proposal_pick(a.std, c);
            const double v = k0 + rr[i] == 0 ? m[i] : ::fma(sd, sE[rr[i] * S + cc[i]], m[i]);   // candidate 0: the plan itself, no noise
            U[e0 + l] = (T)cem_clamp(v, proposal_pick(a.lo, c), proposal_pick(a.hi, c));
        }
    }
}

// One problem: state and seed as kernel arguments, as for mppi_sample_kernel / cem_sample_kernel
struct ProposalSampleArgs {
    rovmpc_state state;                 // written to d_state by block 0 (null d_state: not written)
    double *d_state;
    const double *state_src;            // not null: d_state <- these 16 doubles in device memory instead (first step of a device loop)
    unsigned long long seed;
    ProposalLaw law;
};

template <typename T>
__global__ void __launch_bounds__(PROPOSAL_NT)
proposal_sample_kernel(const ProposalSampleArgs a, T *__restrict__ U) {
    if (a.d_state && blockIdx.x == 0) {
        if (a.state_src) {
            if (threadIdx.x < ROVMPC_STATE_LEN) a.d_state[threadIdx.x] = a.state_src[threadIdx.x];
        } else if (threadIdx.x == 0) {
            // one lane, constant indices: indexing the arguments by the thread would move them all to scratch
            const double *st = reinterpret_cast<const double *>(&a.state);
#pragma unroll
            for (int i = 0; i < ROVMPC_STATE_LEN; ++i) a.d_state[i] = st[i];
        }
    }
    proposal_sample_body<T>(a.seed, a.law, a.law.mean, a.law.sigma, U);
}

// Batched form: blockIdx.y = problem; states and seeds as for mppi_sample_batch_kernel
struct ProposalSampleBatchArgs {
    PlanBatchIn in;
    ProposalLaw law;
};

template <typename T>
__global__ void __launch_bounds__(PROPOSAL_NT)
proposal_sample_batch_kernel(const ProposalSampleBatchArgs a, T *__restrict__ U) {
    const int b = blockIdx.y;
    const unsigned long long seed = plan_batch_seed(a.in, b);
    const size_t off = (size_t)b * 3 * a.law.N;
    proposal_sample_body<T>(seed, a.law, a.law.mean + off, a.law.sigma ? a.law.sigma + off : nullptr,
                            U + (size_t)b * a.law.K * 3 * a.law.N);
}

}  // namespace rovmpc
