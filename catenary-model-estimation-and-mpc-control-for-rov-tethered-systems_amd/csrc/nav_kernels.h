// nav_kernels.h -- the navigation cost of MPPI and CEM on gfx950 (rovmpc_set_nav_cost, rovmpc_nav_cost_device): path
// tracking, terminal, control-rate and keep-out terms of the vehicle's predicted path, added to the costs J[K] between the
// rollout and the update.  The law is stated in include/rovmpc.h above rovmpc_set_nav_cost.  Without a nav cost this kernel
// is not launched.
#pragma once
#include "proposal_kernels.h"

namespace rovmpc {

// C_k reads the 3 N controls of candidate k, which lie one row of U[K][N][3] apart: a thread per candidate would load with a
// stride of 3 N elements.  A workgroup takes a tile of `rows` whole candidates in the form of the shaped sampler
// (proposal_tile() in rovmpc.hip: row stride in LDS 3 N padded up to 3 mod 32, the bank rule worked out in
// proposal_kernels.h) and goes through LDS:
//   1. every thread loads U in element order (coalesced) and stores it as doubles;
//   2. thread t walks (row t / 3, channel t % 3) over n: P_{n+1} = fma(c, U_n, P_n) left in place of U_n, and its channel's
//      position, terminal and rate sums;
//   3. with spheres, a thread per (row, node) forms the node's clearance terms from its three P and leaves their sum in the
//      node's first slot (nobody else reads the three);
//   4. thread t < rows adds row t's clearance terms in node order (slots 3 n of a row: 3 t + 3 n mod 32 over a half-wave, one
//      bank pair each), then the three channel sums and the sphere sum in a fixed order, and updates J_k and / or stores C_k.
// Every row is computed by the same instruction sequence whatever its place in the tile, the tile's place in the problem
// and the problem's place in the batch, so C_k is a function of the row's inputs alone, bit for bit.
constexpr int NAV_NT = 256;
constexpr int NAV_CHUNK = 8;                // nodes whose loads are issued together (phases 2 and 4)

struct NavArgs {
    const double *state;                    // [B][16]: P1 in slots 3..5
    const double *track;                    // [Bt][Tr][3]
    const double *spheres;                  // [n_spheres][4]: cx, cy, cz, R (the handle's device block)
    double *C;                              // [B][K] or null
    double c;                               // v_scale * dt
    double w_pos[3], w_term[3], w_du[3], w_sphere;
    long long K, Tr, r0;                    // r0 = (int64)(step - origin)
    unsigned long long track_stride;        // doubles between the tracks of consecutive problems (0: one track for all)
    int N, rows, stride, n_spheres;         // tile: candidates per workgroup, doubles per tile row in LDS (>= 3 N)
};

// row of the track for node n (1..N): clamp(r0 + n, 0, Tr - 1) without overflow of the sum
RV_DEV long long nav_track_row(long long r0, int n, long long Tr) {
    if (r0 >= Tr) return Tr - 1;
    const long long r = r0 + n;             // r0 < Tr <= 2^24
    return r < 0 ? 0 : (r < Tr ? r : Tr - 1);
}

// Phase 1 of a tile, shared with the tether kernel (tether_kernels.h): the tile's `nel` controls, rows of `row3` elements, in
// element order (coalesced) into LDS rows of stride S as doubles; (r, col) of element l advance with l by NT per pass.
template <typename T, int NT>
RV_DEV void nav_load_tile(const T *__restrict__ Ub, double *sE, int nel, int row3, int S, int tid) {
    const int dr = NT / row3, dc = NT - dr * row3;
    int r = tid / row3, col = tid - r * row3;
    for (int l0 = tid; l0 < nel; l0 += 4 * NT) {
        double u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = l0 + i * NT < nel ? (double)Ub[l0 + i * NT] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (l0 + i * NT < nel) sE[r * S + col] = u[i];
            r += dr; col += dc;
            if (col >= row3) { col -= row3; ++r; }
        }
    }
}

// One node of the vehicle's path, P_{n+1} = fma(c, U_n, P_n): the one statement of it, for both kernels whose laws promise
// the same path bit for bit.
RV_DEV double nav_path_step(double c, double u, double P) { return ::fma(c, u, P); }

template <typename T>
__global__ void __launch_bounds__(NAV_NT)
nav_cost_kernel(const NavArgs a, const T *__restrict__ U, T *__restrict__ J) {
    extern __shared__ __align__(16) unsigned char nav_smem[];
    double *sE = reinterpret_cast<double *>(nav_smem);                      // [rows][stride]
    double *sC = sE + (size_t)a.rows * a.stride;                            // [rows][3]: the channel sums
    const int tid = threadIdx.x, N = a.N, row3 = 3 * N, S = a.stride;
    const size_t b = blockIdx.y;
    const long long k0 = (long long)blockIdx.x * a.rows;
    const int rows = a.K - k0 < a.rows ? (int)(a.K - k0) : a.rows;          // the last tile holds fewer
    const int nel = rows * row3;                                            // <= 4096
    const T *Ub = U + (b * (size_t)a.K + (size_t)k0) * row3;

    // (1) the tile's controls in element order
    nav_load_tile<T, NAV_NT>(Ub, sE, nel, row3, S, tid);
    __syncthreads();

    // (2) one (row, channel) per thread along n: slot n of the row ends up holding P_{n+1}
    for (int t = tid; t < 3 * rows; t += NAV_NT) {
        const int ch = t % 3, row = t / 3;
        double *p = sE + row * S + ch;
        const double wp = proposal_pick(a.w_pos, ch), wt = proposal_pick(a.w_term, ch), wd = proposal_pick(a.w_du, ch);
        const double *ref = a.track + b * a.track_stride + ch;
        double P = a.state[b * ROVMPC_STATE_LEN + 3 + ch];
        double up = 0.0, e = 0.0, s_pos = 0.0, s_du = 0.0;
        for (int n0 = 0; n0 < N; n0 += NAV_CHUNK) {                          // one round trip per chunk, not per node
            double u[NAV_CHUNK], rf[NAV_CHUNK];
#pragma unroll
            for (int i = 0; i < NAV_CHUNK; ++i) {
                const bool in = n0 + i < N;
                u[i] = in ? p[3 * (n0 + i)] : 0.0;
                rf[i] = in ? ref[3 * nav_track_row(a.r0, n0 + i + 1, a.Tr)] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < NAV_CHUNK; ++i) {
                if (n0 + i >= N) break;
                P = nav_path_step(a.c, u[i], P);
                e = P - rf[i];
                s_pos = ::fma(wp, e * e, s_pos);
                if (n0 + i > 0) { const double d = u[i] - up; s_du = ::fma(wd, d * d, s_du); }
                up = u[i];
                p[3 * (n0 + i)] = P;
            }
        }
        sC[3 * row + ch] = (s_pos + wt * (e * e)) + s_du;
    }
    __syncthreads();

    // (3) clearance of node n + 1 of a row from its three P; the sum over the spheres, in their order, into slot 3 n
    if (a.n_spheres > 0) {
        for (int it = tid; it < rows * N; it += NAV_NT) {
            const int row = it / N, n = it - row * N;
            double *p = sE + row * S + 3 * n;
            const double px = p[0], py = p[1], pz = p[2];
            double s = 0.0;
            for (int j = 0; j < a.n_spheres; ++j) {
                const double *sp = a.spheres + 4 * j;
                const double dx = px - sp[0], dy = py - sp[1], dz = pz - sp[2];
                const double g = ::fmax(0.0, sp[3] - ::sqrt(::fma(dx, dx, ::fma(dy, dy, dz * dz))));
                s = ::fma(g, g, s);
            }
            p[0] = s;
        }
        __syncthreads();
    }

    // (4) one thread per row
    if (tid < rows) {
        double s_sph = 0.0;
        if (a.n_spheres > 0) {
            const double *p = sE + tid * S;
            for (int n0 = 0; n0 < N; n0 += NAV_CHUNK) {
                double v[NAV_CHUNK];
#pragma unroll
                for (int i = 0; i < NAV_CHUNK; ++i) v[i] = n0 + i < N ? p[3 * (n0 + i)] : 0.0;
#pragma unroll
                for (int i = 0; i < NAV_CHUNK; ++i) {
                    if (n0 + i >= N) break;
                    s_sph += v[i];
                }
            }
        }
        const double Ck = ((sC[3 * tid] + sC[3 * tid + 1]) + sC[3 * tid + 2]) + a.w_sphere * s_sph;
        const size_t k = b * (size_t)a.K + (size_t)(k0 + tid);
        if (a.C) a.C[k] = Ck;
        if (J) {
            const T j = J[k];
            if (m_finite(j)) J[k] = (T)((double)j + Ck);
        }
    }
}

}  // namespace rovmpc
