// util_kernels.h -- batched mirrors of the reference's per-row helpers (fp64, gfx950).
// Each kernel replaces a Python loop of the reference; see include/rovmpc.h for the map.
#pragma once
#include "rollout_kernels.h"

namespace rovmpc {

// ---- candidate sampler (MPC.step's proposal law, drawn on the GPU) ----------------------------------------------------
// U[k][n][c] = mean[c] + std[c] * z_e, e = (k N + n) 3 + c.  The standard normals are a pure function of (seed, step, e):
// block j = e / 4 is one Philox4x32-10 call (Salmon et al., SC'11; counter (j lo, j hi, step lo, step hi), key (seed lo,
// seed hi)); its four 32-bit outputs x0..x3 give u_i = (x_i + 0.5) 2^-32 and two Box-Muller pairs
// z_{4j}, z_{4j+1} = sqrt(-2 ln u0) (cos, sin)(2 pi u1),  z_{4j+2}, z_{4j+3} = sqrt(-2 ln u2) (cos, sin)(2 pi u3).
// The test oracle restates exactly this law (philox_normals), so a step is reproducible on the host.
// warm != 0: candidate 0 is the previous winner shifted by one step, U[0][n] = Uprev[k*][min(n + 1, N - 1)], k* read
// from the previous record on the device.  The state crosses as a kernel argument (no H2D copy on the step path).
struct SampleArgs {
    rovmpc_state state;                 // written to d_state by block 0 (null d_state: not written)
    double *d_state;
    unsigned long long seed, step;
    double mean[3], std[3];
    long long total;                    // K * N * 3
    int N, warm;
    const void *Uprev;                  // previous candidate tensor (warm start source)
    const double *prev_record;          // previous record: [1] = k*
    const double *warm_seq;             // or: the previous winner's sequence [N][3] itself (then Uprev / prev_record are unused)
};

template <typename T>
__global__ void __launch_bounds__(256)
sample_candidates_kernel(const SampleArgs a, T *__restrict__ U) {
    if (a.d_state && blockIdx.x == 0 && threadIdx.x < ROVMPC_STATE_LEN)
        a.d_state[threadIdx.x] = reinterpret_cast<const double *>(&a.state)[threadIdx.x];
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x, e0 = 4 * j;
    if (e0 >= a.total) return;
    double z[4];
    philox_normal4(a.seed, a.step, j, z);
    const int row3 = 3 * a.N;
    const long long kprev = (a.warm && !a.warm_seq && e0 < row3) ? (long long)a.prev_record[1] : 0;
    const T *Up = reinterpret_cast<const T *>(a.Uprev);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long e = e0 + i;
        if (e >= a.total) break;
        const int c = (int)(e % 3);
        T v = (T)::fma(a.std[c], z[i], a.mean[c]);
        if (a.warm && e < row3) {                       // candidate 0: shifted previous optimum
            const int n = (int)(e / 3), src = n + 1 < a.N ? n + 1 : a.N - 1;
            v = a.warm_seq ? (T)a.warm_seq[3 * src + c] : Up[kprev * row3 + 3 * src + c];
        }
        U[e] = v;
    }
}


// ---- MPPI (rovmpc_mppi_*): sampling around a per-node nominal and the exp(-J/lambda)-weighted update --------------------
// Sampling: U[0] = (T) nu, U[k][n][c] = (T) fma(std[c], z_e, nu[n][c]) for k >= 1, z_e the sampler's stream above with
// `counter` in place of the step (e = (k N + n) 3 + c).  The state crosses as a kernel argument, as for the sampler.
struct MppiSampleArgs {
    rovmpc_state state;                 // written to d_state by block 0 (null d_state: not written)
    double *d_state;
    const double *state_src;            // not null: d_state <- these 16 doubles in device memory instead (first step of a device loop)
    unsigned long long seed, counter;
    double std[3];
    long long total;                    // K * N * 3
    int N;
    const double *nu;                   // nominal [N][3]
};

// the draw of one problem; the batched sampler runs the same body per problem, so the bits are the same
template <typename T>
RV_DEV void mppi_sample_body(unsigned long long seed, unsigned long long counter, const double *std, long long total, int N,
                             const double *nu, T *__restrict__ U) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x, e0 = 4 * j;
    if (e0 >= total) return;
    double z[4];
    philox_normal4(seed, counter, j, z);
    const int row3 = 3 * N;
    int col = (int)(e0 % row3);                         // = 3 n + c
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long e = e0 + i;
        if (e >= total) break;
        const double m = nu[col];
        U[e] = e < row3 ? (T)m : (T)::fma(std[col % 3], z[i], m);
        if (++col == row3) col = 0;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
mppi_sample_kernel(const MppiSampleArgs a, T *__restrict__ U) {
    if (a.d_state && blockIdx.x == 0 && threadIdx.x < ROVMPC_STATE_LEN)
        a.d_state[threadIdx.x] = a.state_src ? a.state_src[threadIdx.x] : reinterpret_cast<const double *>(&a.state)[threadIdx.x];
    mppi_sample_body<T>(a.seed, a.counter, a.std, a.total, a.N, a.nu, U);
}

// Batched form (rovmpc_mppi_step_batch): blockIdx.y = problem.  B states do not fit in the kernel arguments, so the first
// iteration of a control step reads states [B][16] and seeds [B] from one staging block in mapped host memory and block 0
// of each problem keeps them in device memory (d_state, d_seeds) for the step's rollouts and later draws; the later
// iterations read the seeds from there (stage null).  In a device loop (rovmpc_*_closed_loop_batch_device) only the first
// iteration of the first step has a stage, and it takes the seeds alone from it: problem b's state is then row 0 of its exo
// trajectory in device memory (state_src + b * state_src_stride); every later step finds the state its predecessor's last
// update left in d_state (PlanHandoff below).
struct PlanBatchIn {
    const double *stage;                // mapped: states [B][16], then seeds [B]; null after the first iteration
    double *d_state;                    // [B][16]
    unsigned long long *d_seeds;        // [B]
    int B;
    const double *state_src;            // not null: the states come from here (device), not from the stage
    size_t state_src_stride;            // doubles between two problems' rows of state_src
};

RV_DEV unsigned long long plan_batch_seed(const PlanBatchIn &in, int b) {
    if (!in.stage) return in.d_seeds[b];
    const unsigned long long seed = reinterpret_cast<const unsigned long long *>(in.stage + (size_t)in.B * ROVMPC_STATE_LEN)[b];
    if (blockIdx.x == 0) {
        if (threadIdx.x < ROVMPC_STATE_LEN)
            in.d_state[(size_t)b * ROVMPC_STATE_LEN + threadIdx.x] = in.state_src ? in.state_src[(size_t)b * in.state_src_stride + threadIdx.x]
                                                                                  : in.stage[(size_t)b * ROVMPC_STATE_LEN + threadIdx.x];
        if (threadIdx.x == 0) in.d_seeds[b] = seed;
    }
    return seed;
}

struct MppiSampleBatchArgs {
    PlanBatchIn in;
    unsigned long long counter;
    double std[3];
    long long total;                    // K * N * 3 (a problem's share of U)
    int N;
    const double *nu;                   // nominals [B][N][3]
};

template <typename T>
__global__ void __launch_bounds__(256)
mppi_sample_batch_kernel(const MppiSampleBatchArgs a, T *__restrict__ U) {
    const int b = blockIdx.y;
    const unsigned long long seed = plan_batch_seed(a.in, b);
    mppi_sample_body<T>(seed, a.counter, a.std, a.total, a.N, a.nu + (size_t)b * 3 * a.N, U + (size_t)b * a.total);
}

// Update: one read of J[K] and U[K][3N].  Workgroup b takes candidates [b slice, (b + 1) slice) and writes to its slab row
// (rho_b, eta_b, sum w^2_b, S_b[3N]) with rho_b its finite minimum and w = exp(-(J - rho_b) / lambda); the last workgroup to
// take a ticket rescales the rows by exp(-(rho_b - rho) / lambda) and sums them in workgroup order.  Every sum has a fixed
// order (no float atomics), so the result is bitwise reproducible.  Hand-off: wave 0 stores the slab row write-through at
// agent scope and drains its stores before it takes the ticket; the last workgroup reads every slab row with agent-scope
// loads (which bypass the CU's L1), so no cache write-back or invalidate is needed on either side.
constexpr int MPPI_NT = 256;                // threads of the update kernel
constexpr int MPPI_MAX_COLS = 1024;         // 3 N (N < 341)
constexpr int MPPI_ROWS_PER_WG = 64;        // candidates per workgroup, until the grid reaches MPPI_MAX_WG
constexpr int MPPI_MAX_WG = MPPI_NT;        // the combine reads one slab row per thread

// Loop hand-off of a control step's last update (rovmpc_*_closed_loop*_device; row null: off, as in every single step).
// Wave 0 of the finishing workgroup, which fills the mailbox, also writes the same row to `row` in device memory and turns
// `state` into the next step's by plant_update_kernel's rule: slots 0..11 (feedback 0: 0..15) from the next measured row,
// and with feedback (theta_prev, gamma_prev) <- (theta, gamma), (theta, gamma) <- record[7], record[8], the first predicted
// node of this step's last rollout's cheapest candidate.  Plain stores: the step's rollouts are over (stream order), the
// next sampler does not read the state, and the next rollout is a later launch on the same stream.  Problem b of a batch
// lies b strides behind problem 0 (its state: b * 16).
struct PlanHandoff {
    double *row;                        // this step's row of d_rows
    const double *exo_next;             // the next step's measured row [16], or null at the last step (state is left alone)
    double *state;                      // the controller's device state [16]
    int feedback;
    size_t row_stride, exo_stride;      // doubles per problem
};

// by whole wave 0, after the record's u has been written
RV_DEV void plan_handoff_state(const PlanHandoff &lp, size_t b, const double *record) {
    if (!lp.exo_next) return;
    const int lane = threadIdx.x & 63;
    const double *nx = lp.exo_next + b * lp.exo_stride;
    double *st = lp.state + b * ROVMPC_STATE_LEN;
    if (lane < (lp.feedback ? 12 : ROVMPC_STATE_LEN)) {
        st[lane] = nx[lane];
    } else if (lp.feedback && lane == 12) {
        const double th = st[12], ga = st[13];
        st[14] = th; st[15] = ga;
        st[12] = record[7]; st[13] = record[8];
    }
}

struct MppiUpdateArgs {
    const void *J, *U;                  // T [K], T [K][3N]
    long long K, slice;                 // candidates, candidates per workgroup
    int C3, G;                          // 3 N, workgroups
    double lambda;
    const double *nu_in;                // [3N]
    double *nu_out;                     // [3N]: nu_{i+1}, or with shift != 0 the kept nominal nu[n] = nu*[min(n + 1, N - 1)]
    int shift;
    double *stats;                      // [4] (rho, eta, ESS, J_0) or null
    double *slab;                       // [G][3 + 3N]
    unsigned *ticket;                   // 0 between launches (the last workgroup re-arms it)
    // last iteration of a control step (null record: none): u of the device record <- nu*[0]; then host_out (mapped) =
    // [record (R), nu* (3N), stats (4)] and done_seq released into *done_flag at system scope
    double *record;
    int R;
    double *host_out;
    unsigned long long *done_flag, done_seq;
    // a step of a device loop: the row also goes to loop.row, the state moves on, and only the loop's last step has a
    // mailbox (host_out and done_flag null otherwise)
    PlanHandoff loop;
    double lo[3], hi[3];                // the box of rovmpc_mppi_set_bounds (read by the bounded instances only)
};

RV_DEV double wave_min(double v) {
    for (int off = 32; off > 0; off >>= 1) v = ::fmin(v, __shfl_xor(v, off, 64));
    return v;
}
RV_DEV double wave_sum(double v) {          // butterfly: every lane ends with the same bits
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

constexpr int MPPI_CHUNK = 8;             // rows (slab rows in the combine) whose loads are issued together

// Publication of a control step's last update.  One problem: the finishing workgroup's wave 0 has written the mailbox and
// releases done_seq at system scope.  A batch (step_ticket not null): each problem's finishing workgroup has written its own
// mailbox row; it releases the row and takes the step's ticket, and the last of the B acquires the others' rows through
// that ticket before it releases done_seq, so the host never reads a row that is not yet visible.  Called by whole wave 0.
RV_DEV void plan_publish(unsigned long long *done_flag, unsigned long long done_seq, unsigned *step_ticket, int B) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if ((threadIdx.x & 63) != 0) return;
    if (step_ticket) {
        if (__hip_atomic_fetch_add(step_ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM) != (unsigned)(B - 1)) return;
        __hip_atomic_store(step_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // re-armed for the next step
    }
    __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Where a workgroup's problem lies behind problem 0 of the arguments (all zero: a single-problem launch)
struct PlanBatchAt {
    size_t b = 0;                       // problem
    size_t slab_stride = 0, host_stride = 0;   // 64-bit words per problem of the slab and of the mailbox
    unsigned *step_ticket = nullptr;    // of the batch's last iteration (plan_publish)
    int B = 0;
};

// The update of one problem by the workgroups blockIdx.x = 0 .. G - 1 (the kernels below: one problem, or blockIdx.y = problem).
// QC = columns per thread: 1 when 3 N <= MPPI_NT, else 4.  BOX: every nu the update leaves goes through the box [a.lo, a.hi]
// (fmin(fmax(.)) as cem_clamp), the row it keeps when no cost is finite included; the unbounded instances carry no selects.
template <typename T, int QC, bool BOX = false>
RV_DEV void mppi_update_body(const MppiUpdateArgs &a, const PlanBatchAt &at) {
    __shared__ double sS[MPPI_MAX_COLS];                // row-lane partials [R][3N]
    __shared__ double sNu[MPPI_MAX_COLS];               // nu* (combine)
    __shared__ double sScale[MPPI_MAX_WG], sW[MPPI_NT], sEta[4], sW2[4];
    __shared__ double sRed[16];
    __shared__ int sLast;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const T *__restrict__ J = static_cast<const T *>(a.J) + at.b * a.K;
    const T *__restrict__ U = static_cast<const T *>(a.U) + at.b * a.K * a.C3;
    const int C3 = a.C3, G = a.G;
    // the problem's other arrays, each taken from the arguments where it is used
    auto nu_in = [&] { return a.nu_in + at.b * C3; };
    auto nu_out = [&] { return a.nu_out + at.b * C3; };
    auto slab_p = [&] { return a.slab + at.b * at.slab_stride; };
    auto ticket = [&] { return a.ticket + at.b; };
    // threads map to columns so that each candidate row is one coalesced read; R rows side by side when 3N <= 256,
    // otherwise one row with up to four columns per thread
    const int R = C3 <= MPPI_NT ? MPPI_NT / C3 : 1;
    const int r = C3 <= MPPI_NT ? tid / C3 : 0, c0 = C3 <= MPPI_NT ? tid - r * C3 : tid;
    const bool active = r < R;
    const long long k0 = (long long)blockIdx.x * a.slice, k1 = k0 + a.slice < a.K ? k0 + a.slice : a.K;
    const double inf = __builtin_inf();
    auto box = [&](double v, int c) { return BOX ? ::fmin(::fmax(v, a.lo[c % 3]), a.hi[c % 3]) : v; };

    // (1) the workgroup's finite minimum
    double m = inf;
    for (long long k = k0 + tid; k < k1; k += MPPI_NT) {
        const double v = (double)J[k];
        if (::isfinite(v) && v < m) m = v;
    }
    m = wave_min(m);
    if (lane == 0) sRed[wv] = m;
    __syncthreads();
    const double rho_b = ::fmin(::fmin(sRed[0], sRed[1]), ::fmin(sRed[2], sRed[3]));

    // (2) weights, a tile of MPPI_NT rows at a time: one lane per row computes w into LDS, then row-lane r takes rows
    //     r, r + R, ... of the tile in order, the loads of MPPI_CHUNK rows issued before any of them is used
    double S[4] = {0.0, 0.0, 0.0, 0.0}, eta = 0.0, w2 = 0.0;
    for (long long kt = k0; kt < k1; kt += MPPI_NT) {
        double w = 0.0;
        if (kt + tid < k1) {
            const double v = (double)J[kt + tid];
            if (::isfinite(v)) w = ::exp(-(v - rho_b) / a.lambda);
        }
        eta += w;
        w2 = ::fma(w, w, w2);
        sW[tid] = w;
        __syncthreads();
        const int nrow = k1 - kt < MPPI_NT ? (int)(k1 - kt) : MPPI_NT;
        if (active) {
            for (int jb = r; jb < nrow; jb += MPPI_CHUNK * R) {
                double uv[MPPI_CHUNK][QC];
#pragma unroll
                for (int t = 0; t < MPPI_CHUNK; ++t) {
                    const int j = jb + t * R;
#pragma unroll
                    for (int q = 0; q < QC; ++q) {
                        const int c = c0 + q * MPPI_NT;
                        uv[t][q] = (j < nrow && c < C3) ? (double)U[(kt + j) * C3 + c] : 0.0;
                    }
                }
#pragma unroll
                for (int t = 0; t < MPPI_CHUNK; ++t) {
                    const int j = jb + t * R;
                    const double wj = j < nrow ? sW[j] : 0.0;
                    if (wj == 0.0) continue;              // not finite (or underflowed): contributes nothing
#pragma unroll
                    for (int q = 0; q < QC; ++q) S[q] = ::fma(wj, uv[t][q], S[q]);
                }
            }
        }
        __syncthreads();
    }
    eta = wave_sum(eta);
    w2 = wave_sum(w2);
    if (lane == 0) { sEta[wv] = eta; sW2[wv] = w2; }
    if (C3 <= MPPI_NT) {
        if (active) sS[r * C3 + c0] = S[0];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (c0 + q * MPPI_NT < C3) sS[c0 + q * MPPI_NT] = S[q];
    }
    __syncthreads();

    // (3) wave 0 sums the row-lanes in order, stores the slab row write-through and takes the ticket
    if (wv == 0) {
        double *slab = slab_p() + (size_t)blockIdx.x * (3 + C3);
        for (int c = lane; c < C3; c += 64) {
            double s = sS[c];
            for (int q = 1; q < R; ++q) s += sS[q * C3 + c];
            st_agent(slab + 3 + c, s);
        }
        if (lane == 0) {
            st_agent(slab, rho_b);
            st_agent(slab + 1, ((sEta[0] + sEta[1]) + sEta[2]) + sEta[3]);
            st_agent(slab + 2, ((sW2[0] + sW2[1]) + sW2[2]) + sW2[3]);
        }
        // write-through stores acknowledged before the ticket that announces them (no L2 write-back fence needed)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) sLast = __hip_atomic_fetch_add(ticket(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(G - 1);
    }
    __syncthreads();
    if (!sLast) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: keeps the slab loads below the ticket)

    // (4) combine (last workgroup)
    if (tid == 0) __hip_atomic_store(ticket(), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double rb = inf, eb = 0.0, wb = 0.0;
    if (tid < G) {
        const double *s = slab_p() + (size_t)tid * (3 + C3);
        rb = ld_agent(s); eb = ld_agent(s + 1); wb = ld_agent(s + 2);
    }
    m = wave_min(rb);
    if (lane == 0) sRed[4 + wv] = m;
    __syncthreads();
    const double rho = ::fmin(::fmin(sRed[4], sRed[5]), ::fmin(sRed[6], sRed[7]));
    const double J0 = (double)J[0];
    double st0, st1, st2;
    if (!(rho < inf)) {
        // no finite cost: the nominal stays as it is, bit for bit
        for (int c = tid; c < C3; c += MPPI_NT) sNu[c] = box(nu_in()[c], c);
        st0 = __builtin_nan(""); st1 = 0.0; st2 = 0.0;
    } else {
        const double sc = (tid < G && rb < inf) ? ::exp(-(rb - rho) / a.lambda) : 0.0;
        sScale[tid] = sc;
        const double e = wave_sum(sc * eb), w = wave_sum(sc * sc * wb);
        if (lane == 0) { sRed[8 + wv] = e; sRed[12 + wv] = w; }
        __syncthreads();
        const double eta_all = ((sRed[8] + sRed[9]) + sRed[10]) + sRed[11];
        const double w2_all = ((sRed[12] + sRed[13]) + sRed[14]) + sRed[15];
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (active) {
            for (int bb = r; bb < G; bb += MPPI_CHUNK * R) {
                double sv[MPPI_CHUNK][QC];
#pragma unroll
                for (int t = 0; t < MPPI_CHUNK; ++t) {
                    const int b = bb + t * R;
                    const double *row = slab_p() + (size_t)b * (3 + C3) + 3;
#pragma unroll
                    for (int q = 0; q < QC; ++q) {
                        const int c = c0 + q * MPPI_NT;
                        sv[t][q] = (b < G && c < C3) ? ld_agent(row + c) : 0.0;
                    }
                }
#pragma unroll
                for (int t = 0; t < MPPI_CHUNK; ++t) {
                    const int b = bb + t * R;
                    const double s = b < G ? sScale[b] : 0.0;
                    if (s == 0.0) continue;
#pragma unroll
                    for (int q = 0; q < QC; ++q) acc[q] = ::fma(s, sv[t][q], acc[q]);
                }
            }
        }
        if (C3 <= MPPI_NT) {
            if (active) sS[r * C3 + c0] = acc[0];
            __syncthreads();
            if (tid < C3) {
                double s = sS[tid];
                for (int q = 1; q < R; ++q) s += sS[q * C3 + tid];
                sNu[tid] = box(s / eta_all, tid);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (c0 + q * MPPI_NT < C3) sNu[c0 + q * MPPI_NT] = box(acc[q] / eta_all, c0 + q * MPPI_NT);
        }
        st0 = rho; st1 = eta_all; st2 = eta_all * eta_all / w2_all;
    }
    __syncthreads();
    for (int c = tid; c < C3; c += MPPI_NT) nu_out()[c] = sNu[a.shift && c + 3 < C3 ? c + 3 : c];
    if (a.stats && tid == 0) { a.stats[0] = st0; a.stats[1] = st1; a.stats[2] = st2; a.stats[3] = J0; }
    if (a.record && wv == 0) {
        // the control to apply is nu*[0]; the rest of the record is the rollout's
        double *record = a.record + at.b * a.R;
        if (lane < 3) record[2 + lane] = sNu[lane];
        auto row_to = [&](double *o) {
            for (int i = lane; i < a.R; i += 64) o[i] = (i >= 2 && i < 5) ? sNu[i - 2] : record[i];
            for (int c = lane; c < C3; c += 64) o[a.R + c] = sNu[c];
            if (lane == 0) { o[a.R + C3] = st0; o[a.R + C3 + 1] = st1; o[a.R + C3 + 2] = st2; o[a.R + C3 + 3] = J0; }
        };
        if (a.loop.row) {
            row_to(a.loop.row + at.b * a.loop.row_stride);
            plan_handoff_state(a.loop, at.b, record);
        }
        if (a.host_out) {
            row_to(a.host_out + at.b * at.host_stride);
            plan_publish(a.done_flag, a.done_seq, at.step_ticket, at.B);
        }
    }
}

template <typename T, int QC>
__global__ void __launch_bounds__(MPPI_NT)
mppi_update_kernel(const MppiUpdateArgs a) {
    mppi_update_body<T, QC>(a, PlanBatchAt{});
}

// the bounded instance (rovmpc_mppi_set_bounds with a finite bound)
template <typename T, int QC>
__global__ void __launch_bounds__(MPPI_NT)
mppi_update_box_kernel(const MppiUpdateArgs a) {
    mppi_update_body<T, QC, true>(a, PlanBatchAt{});
}

// Batched form: grid (G, B).  Problem b = blockIdx.y has its own J, U, nominal halves, slab rows, ticket, record and mailbox
// row, each at the first problem's pointer + b * its stride (PlanBatchAt); within a problem everything is mppi_update_body.
struct MppiUpdateBatchArgs {
    MppiUpdateArgs a;                   // problem 0
    size_t slab_stride, host_stride;    // doubles per problem
    unsigned *step_ticket;              // last iteration: 0 between steps
    int B;
};

template <typename T, int QC>
__global__ void __launch_bounds__(MPPI_NT)
mppi_update_batch_kernel(const MppiUpdateBatchArgs ba) {
    mppi_update_body<T, QC>(ba.a, PlanBatchAt{blockIdx.y, ba.slab_stride, ba.host_stride, ba.step_ticket, ba.B});
}

template <typename T, int QC>
__global__ void __launch_bounds__(MPPI_NT)
mppi_update_box_batch_kernel(const MppiUpdateBatchArgs ba) {
    mppi_update_body<T, QC, true>(ba.a, PlanBatchAt{blockIdx.y, ba.slab_stride, ba.host_stride, ba.step_ticket, ba.B});
}

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
            it = k1t * dt; ig = k1g * dt;
        } else {
            for (int f = 0; f < F; ++f) feat[(size_t)f * NT] = (x0[f] + x1[f]) / 2;   // :62-63
            const double k2t = interp_eval<double>(code_th, n_th, consts, feat, NT, stack, NT);
            const double k2g = interp_eval<double>(code_ga, n_ga, consts, feat, NT, stack, NT);
            const double k4t = interp_eval<double>(code_th, n_th, consts, x1, 1, stack, NT);
            const double k4g = interp_eval<double>(code_ga, n_ga, consts, x1, 1, stack, NT);
            it = (dt / 6) * (k1t + 2 * k2t + 2 * k2t + k4t);                          // :66
            ig = (dt / 6) * (k1g + 2 * k2g + 2 * k2g + k4g);
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
        if (integrator == ROVMPC_DOUBLE_EULER) {
            y = y + v * dt;
            v = v + dd[i - 1] * dt;
        } else {
            v = v + (dd[i - 1] + dd[i]) / 2 * dt;
            y = y + dt * v;
        }
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

// ---- placement probe of the collective streams (rovmpc.hip::place_comm_streams) ------------------------------------------
// A kernel that waits on one hardware queue can hold back the COMPLETION of kernels on another queue of the same
// command-processor pipe (queues k and k + 4 share one; tools/ubench/queue_collision.hip: +24 us per kernel).  The probe
// reproduces that on purpose: one lane parks on the candidate stream until `raise` (last on the caller's stream) lets it go
// or 2 ms pass; meanwhile a few short grids run back to back on the caller's stream.
__global__ void __launch_bounds__(64)
probe_park_kernel(const unsigned long long *flag, unsigned long long want, unsigned long long ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long give_up = wall_clock64() + ticks;
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        if (wall_clock64() > give_up) break;
        __builtin_amdgcn_s_sleep(16);
    }
}
__global__ void __launch_bounds__(64)
probe_short_kernel(double *x) {
    double v = x[blockIdx.x * 64 + threadIdx.x];
#pragma unroll 1
    for (int i = 0; i < 256; ++i) v = __builtin_fma(v, 1.0000001, 1e-9);
    x[blockIdx.x * 64 + threadIdx.x] = v;
}
__global__ void probe_raise_kernel(unsigned long long *flag, unsigned long long v) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
