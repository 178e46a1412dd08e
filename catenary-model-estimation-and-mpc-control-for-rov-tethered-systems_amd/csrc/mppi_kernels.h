// mppi_kernels.h -- the candidate sampler, the MPPI kernels and what the plan controllers (MPPI, CEM) share (fp64 plans, gfx950).
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

}  // namespace rovmpc
