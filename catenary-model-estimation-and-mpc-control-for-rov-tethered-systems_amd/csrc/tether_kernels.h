// tether_kernels.h -- the tether keep-out cost of MPPI and CEM on gfx950 (rovmpc_set_tether_cost, rovmpc_tether_cost_device):
// the squared penetration of the augmented catenary cable of every predicted node into up to 8 spheres, added to the costs
// J[K] between the rollout (and the navigation cost, if any) and the update.  The law is stated in include/rovmpc.h above
// rovmpc_set_tether_cost.  Without a tether cost this kernel is not launched.
#pragma once
#include "nav_kernels.h"

namespace rovmpc {

// A workgroup takes a tile of `rows` whole candidates (4: a tile holds rows x N cable solves, the work that counts, and small
// tiles give every CU several workgroups whose fp64 chains overlap) with the LDS row stride of the shaped sampler
// (proposal_tile() in rovmpc.hip) and goes through LDS:
//   1. every thread loads U in element order (coalesced) and stores it as doubles: nav_load_tile of nav_kernels.h;
//   2. thread t walks (row t / 3, channel t % 3) over n by nav_path_step, the navigation kernel's statement of the path:
//      slot n ends up holding P_{n+1};
//   then, for chunks of `nc` nodes (rows x nc x M x 3 doubles of cable points must fit in LDS beside the tile):
//   3. a thread per (row, node): axes, the theta-rotated end point, ONE catenary solve, and the node's TETHER_PAR parameters
//      into LDS;
//   4. a thread per (row, node, sample): the sample, turned back by -theta and by gamma, into LDS as X - A;
//   5. a thread per (row, node, sphere): the minimum over the M - 1 segments of the squared point-to-segment distance (a
//      minimum is exact in any order; sqrt is monotone, so one sqrt of the minimum), then the penetration and the clearance
//      into the node's parameter slots (nobody reads the parameters any more);
//   6. a thread per (row, node) writes D; thread t < rows adds row t's penetrations in node order, then sphere order, into a
//      register it keeps across the chunks.
// Every (row, node) is computed by the same instruction sequence whatever its place in the tile, the chunk and the batch,
// so C_k and D_k are functions of the row's inputs alone, bit for bit.
constexpr int TETHER_NT = 256;
constexpr int TETHER_ROWS = 4;
constexpr int TETHER_PAR = 20;              // doubles per (row, node): see tether_node below (>= 2 x ROVMPC_TETHER_MAX_SPHERES)

struct TetherArgs {
    const double *state;                    // [B][16]: P0 in slots 0..2, P1 in slots 3..5
    const double *spheres;                  // [n_spheres][4]: cx, cy, cz, R (the handle's device block)
    double *C;                              // [B][K] or null
    double *D;                              // [B][K][N] or null
    double c;                               // v_scale * dt
    double w, margin, L, c_lo, c_hi, up;    // L, c_lo, c_hi rounded to the handle's dtype, as the rollout holds them
    long long K;
    int N, M, rows, stride, nc, n_spheres;  // tile rows, doubles per tile row in LDS (>= 3 N), nodes per chunk
};

// parameter slots of one (row, node)
enum { TP_FLAG = 0, TP_BX, TP_BY, TP_U, TP_ATH, TP_2IC, TP_KTX, TP_KTY, TP_ST, TP_CT, TP_KGX, TP_KGY, TP_KGZ, TP_SG, TP_CG,
       TP_RX, TP_RY, TP_RZ };               // TP_FLAG: 1 catenary, 0 chord, NaN non-finite node

// phase 3 for one node: rel = P_n - A and (theta, gamma) to the node's parameters
RV_DEV void tether_node(const TetherArgs &a, V3<double> rel, double th, double ga, double *par) {
    V3<double> kt, kg;
    theta_gamma_axes(rel, kt, kg);
    double st, ct, sg, cg;
    m_sincos(th, &st, &ct);
    m_sincos(ga, &sg, &cg);
    const V3<double> Bp = rodrigues_unit(rel, kt, st, ct);
    const double lp = m_sqrtq(Bp.x * Bp.x + Bp.y * Bp.y), dHp = a.up * Bp.z;
    const CatRoot<double> root = solve_catenary_root(lp, dHp, a.L, a.c_lo, a.c_hi);
    const bool valid = root.C == root.C;
    // a non-finite angle or gamma axis (rel = 0) makes every point of the node non-finite, on the chord too: the reference
    // turns the chord's end point by the same two rotations
    const double chk = ((th - th) + (ga - ga)) + ((kg.x - kg.x) + (kg.y - kg.y) + (kg.z - kg.z));
    par[TP_FLAG] = chk != chk ? chk : (valid ? 1.0 : 0.0);
    par[TP_BX] = Bp.x; par[TP_BY] = Bp.y;
    par[TP_U] = root.u;
    par[TP_ATH] = valid ? m_atanh(dHp / a.L) : 0.0;
    par[TP_2IC] = valid ? 2.0 / root.C : 0.0;
    par[TP_KTX] = kt.x; par[TP_KTY] = kt.y; par[TP_ST] = st; par[TP_CT] = ct;
    par[TP_KGX] = kg.x; par[TP_KGY] = kg.y; par[TP_KGZ] = kg.z; par[TP_SG] = sg; par[TP_CG] = cg;
    par[TP_RX] = rel.x; par[TP_RY] = rel.y; par[TP_RZ] = rel.z;
}

// phase 4 for one sample: X_{n,m} - A.  With C' x0 = u' - atanh(dH'/L) the sample's height is
//   (cosh(C'(l' t - x0)) - cosh(C' x0)) / C' = 2 sinh(u' t) sinh(u' (t - 1) + atanh(dH'/L)) / C':
// the same value without the cancellation of two cosh near 1, exactly 0 at t = 0.
RV_DEV V3<double> tether_sample(const TetherArgs &a, const double *par, int m) {
    const double t = (double)m / (double)(a.M - 1);         // exactly 1 at the far end
    const double flag = par[TP_FLAG];
    if (flag != flag) return {flag, flag, flag};
    if (flag == 0.0) return {t * par[TP_RX], t * par[TP_RY], t * par[TP_RZ]};
    const double u = par[TP_U];
    const double s = par[TP_2IC] * (m_sinh(u * t) * m_sinh(::fma(u, t - 1.0, par[TP_ATH])));
    V3<double> q = {t * par[TP_BX], t * par[TP_BY], a.up * s};
    q = rodrigues_unit(q, V3<double>{par[TP_KTX], par[TP_KTY], 0.0}, -par[TP_ST], par[TP_CT]);
    return rodrigues_unit(q, V3<double>{par[TP_KGX], par[TP_KGY], par[TP_KGZ]}, par[TP_SG], par[TP_CG]);
}

template <typename T>
__global__ void __launch_bounds__(TETHER_NT)
tether_cost_kernel(const TetherArgs a, const T *__restrict__ U, const T *__restrict__ traj, T *__restrict__ J) {
    extern __shared__ __align__(16) unsigned char tether_smem[];
    const int tid = threadIdx.x, N = a.N, M = a.M, row3 = 3 * N, S = a.stride, NC = a.nc;
    double *sE = reinterpret_cast<double *>(tether_smem);                   // [rows][stride]
    double *sPar = sE + (size_t)a.rows * S;                                 // [rows][NC][TETHER_PAR]
    double *sX = sPar + (size_t)a.rows * NC * TETHER_PAR;                   // [rows][NC][M][3]
    const size_t b = blockIdx.y;
    const long long k0 = (long long)blockIdx.x * a.rows;
    const int rows = a.K - k0 < a.rows ? (int)(a.K - k0) : a.rows;          // the last tile holds fewer
    const int nel = rows * row3;
    const size_t kb = b * (size_t)a.K + (size_t)k0;                         // the tile's first candidate among B K
    const T *Ub = U + kb * row3;
    const T *trajb = traj + kb * (size_t)(N + 1) * 2;

    // (1) the tile's controls in element order: the navigation kernel's load
    nav_load_tile<T, TETHER_NT>(Ub, sE, nel, row3, S, tid);
    __syncthreads();

    // (2) one (row, channel) per thread along n: slot n of the row ends up holding P_{n+1}
    if (tid < 3 * rows) {
        const int ch = tid % 3, row = tid / 3;
        double *p = sE + row * S + ch;
        double P = a.state[b * ROVMPC_STATE_LEN + 3 + ch];
        for (int n0 = 0; n0 < N; n0 += NAV_CHUNK) {                          // one round trip per chunk, not per node
            double u[NAV_CHUNK];
#pragma unroll
            for (int i = 0; i < NAV_CHUNK; ++i) u[i] = n0 + i < N ? p[3 * (n0 + i)] : 0.0;
#pragma unroll
            for (int i = 0; i < NAV_CHUNK; ++i) {
                if (n0 + i >= N) break;
                P = nav_path_step(a.c, u[i], P);
                p[3 * (n0 + i)] = P;
            }
        }
    }
    __syncthreads();

    const double Ax = a.state[b * ROVMPC_STATE_LEN], Ay = a.state[b * ROVMPC_STATE_LEN + 1], Az = a.state[b * ROVMPC_STATE_LEN + 2];
    double acc = 0.0;                       // thread t < rows: row t's sum of squared penetrations, and whether a node was
    bool bad = false;                       // non-finite
    for (int n0 = 0; n0 < N; n0 += NC) {
        const int nc = N - n0 < NC ? N - n0 : NC, items = rows * nc;

        // (3) one solve per (row, node); consecutive items go to different waves, so a chunk with fewer items than threads
        // (80 at N = 20) keeps all four SIMDs busy instead of two
        for (int i0 = 0; i0 < items; i0 += TETHER_NT) {
            const int it = i0 + (tid & 63) * (TETHER_NT / 64) + (tid >> 6);
            if (it >= items) continue;
            const int row = it / nc, n = n0 + (it - row * nc);              // node n + 1 of the law
            const double *p = sE + row * S + 3 * n;
            const T *tg = trajb + ((size_t)row * (N + 1) + (n + 1)) * 2;
            tether_node(a, V3<double>{p[0] - Ax, p[1] - Ay, p[2] - Az}, (double)tg[0], (double)tg[1], sPar + (size_t)it * TETHER_PAR);
        }
        __syncthreads();

        // (4) the samples
        for (int is = tid; is < items * M; is += TETHER_NT) {
            const int it = is / M, m = is - it * M;
            const V3<double> x = tether_sample(a, sPar + (size_t)it * TETHER_PAR, m);
            double *o = sX + (size_t)is * 3;
            o[0] = x.x; o[1] = x.y; o[2] = x.z;
        }
        __syncthreads();

        // (5) distance of sphere j to the cable of (row, node); all relative to A
        for (int ij = tid; ij < items * a.n_spheres; ij += TETHER_NT) {
            const int it = ij / a.n_spheres, j = ij - it * a.n_spheres;
            const double *sp = a.spheres + 4 * j;
            const double cx = sp[0] - Ax, cy = sp[1] - Ay, cz = sp[2] - Az, rm = sp[3] + a.margin;
            const double *x = sX + (size_t)it * M * 3;
            double ax = x[0], ay = x[1], az = x[2];
            double fin = (ax - ax) + (ay - ay) + (az - az);                 // 0, or NaN once a point is non-finite
            double d2 = __builtin_inf();
            for (int m = 1; m < M; ++m) {
                const double bx = x[3 * m], by = x[3 * m + 1], bz = x[3 * m + 2];
                fin += (bx - bx) + (by - by) + (bz - bz);
                const double ex = bx - ax, ey = by - ay, ez = bz - az;
                const double px = cx - ax, py = cy - ay, pz = cz - az;
                const double den = ::fma(ex, ex, ::fma(ey, ey, ez * ez));
                double ts = den > 0.0 ? ::fma(px, ex, ::fma(py, ey, pz * ez)) / den : 0.0;
                ts = ts < 0.0 ? 0.0 : (ts > 1.0 ? 1.0 : ts);
                const double qx = ::fma(-ts, ex, px), qy = ::fma(-ts, ey, py), qz = ::fma(-ts, ez, pz);
                d2 = ::fmin(d2, ::fma(qx, qx, ::fma(qy, qy, qz * qz)));
                ax = bx; ay = by; az = bz;
            }
            const double d = ::sqrt(d2);
            const double pen = ::fmax(0.0, rm - d);
            double *par = sPar + (size_t)it * TETHER_PAR;
            par[j] = fin != fin ? fin : pen * pen;
            par[ROVMPC_TETHER_MAX_SPHERES + j] = fin != fin ? fin : d - rm;
        }
        __syncthreads();

        // (6) D of the chunk's nodes; the row's sum in node order, then sphere order
        if (a.D) {
            for (int it = tid; it < items; it += TETHER_NT) {
                const int row = it / nc, n = n0 + (it - row * nc);
                const double *par = sPar + (size_t)it * TETHER_PAR + ROVMPC_TETHER_MAX_SPHERES;
                double dmin = par[0];
                for (int j = 1; j < a.n_spheres; ++j) { const double v = par[j]; dmin = (v != v || v < dmin) ? v : dmin; }
                a.D[(kb + row) * (size_t)N + n] = dmin;
            }
        }
        if (tid < rows) {
            const double *par = sPar + (size_t)tid * nc * TETHER_PAR;
            for (int nl = 0; nl < nc; ++nl)
                for (int j = 0; j < a.n_spheres; ++j) {
                    const double v = par[nl * TETHER_PAR + j];
                    if (v != v) bad = true; else acc += v;
                }
        }
        __syncthreads();                    // the next chunk writes the parameters
    }

    if (tid < rows) {
        const double Ck = bad ? __builtin_inf() : a.w * acc;
        const size_t k = kb + tid;
        if (a.C) a.C[k] = Ck;
        if (J) {
            const T j = J[k];
            if (m_finite(j)) J[k] = (T)((double)j + Ck);
        }
    }
}

}  // namespace rovmpc
