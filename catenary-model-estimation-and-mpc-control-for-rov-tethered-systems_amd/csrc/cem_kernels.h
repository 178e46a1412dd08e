// cem_kernels.h -- the cross-entropy method (rovmpc_cem_*) on gfx950: clamped sampling around a per-node mean with a per-node
// spread, and one launch that selects the n_elite cheapest candidates exactly and refits mean and spread from them.
// The law is stated in include/rovmpc.h above rovmpc_cem_params.
#pragma once
#include "mppi_kernels.h"

namespace rovmpc {

RV_DEV double cem_clamp(double v, double lo, double hi) { return ::fmin(::fmax(v, lo), hi); }

// ---- sampling: U[0] = (T) clamp(mu), U[k][n][c] = (T) clamp(fma(sigma[n][c], z_e, mu[n][c])) for k >= 1 ----------------------
// z_e is the sampler's stream (philox_normal4) keyed by (seed, counter), e = (k N + n) 3 + c, as for mppi_sample_kernel.
struct CemSampleArgs {
    rovmpc_state state;                 // written to d_state by block 0 (null d_state: not written)
    double *d_state;
    const double *state_src;            // not null: d_state <- these 16 doubles in device memory instead (first step of a device loop)
    unsigned long long seed, counter;
    double std[3], lo[3], hi[3];
    long long total;                    // K * N * 3
    int N;
    const double *mu;                   // [N][3]
    const double *sigma;                // [N][3], or null: std[c] on every node
};

// the draw of one problem; the batched sampler runs the same body per problem, so the bits are the same
template <typename T>
RV_DEV void cem_sample_body(unsigned long long seed, unsigned long long counter, const double *std, const double *lo,
                            const double *hi, long long total, int N, const double *mu, const double *sigma, T *__restrict__ U) {
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
        const int c = col % 3;
        const double m = mu[col], s = sigma ? sigma[col] : std[c];
        U[e] = (T)cem_clamp(e < row3 ? m : ::fma(s, z[i], m), lo[c], hi[c]);
        if (++col == row3) col = 0;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
cem_sample_kernel(const CemSampleArgs a, T *__restrict__ U) {
    if (a.d_state && blockIdx.x == 0 && threadIdx.x < ROVMPC_STATE_LEN)
        a.d_state[threadIdx.x] = a.state_src ? a.state_src[threadIdx.x] : reinterpret_cast<const double *>(&a.state)[threadIdx.x];
    cem_sample_body<T>(a.seed, a.counter, a.std, a.lo, a.hi, a.total, a.N, a.mu, a.sigma, U);
}

// Batched form (rovmpc_cem_step_batch): blockIdx.y = problem; states and seeds as for mppi_sample_batch_kernel.
struct CemSampleBatchArgs {
    PlanBatchIn in;
    unsigned long long counter;
    double std[3], lo[3], hi[3];
    long long total;                    // K * N * 3 (a problem's share of U)
    int N;
    const double *mu;                   // [B][N][3]
    const double *sigma;                // [B][N][3], or null: std[c] on every node
};

template <typename T>
__global__ void __launch_bounds__(256)
cem_sample_batch_kernel(const CemSampleBatchArgs a, T *__restrict__ U) {
    const int b = blockIdx.y;
    const unsigned long long seed = plan_batch_seed(a.in, b);
    const size_t off = (size_t)b * 3 * a.N;
    cem_sample_body<T>(seed, a.counter, a.std, a.lo, a.hi, a.total, a.N, a.mu + off, a.sigma ? a.sigma + off : nullptr,
                       U + (size_t)b * a.total);
}

// ---- selection and refit ------------------------------------------------------------------------------------------------
// Costs map to order-preserving 64-bit keys (cem_key); the order of candidates is that of the pairs (key, k), so ties go to
// the lower index, and non-finite costs are no candidates.  Workgroup b takes candidates [b slice, (b + 1) slice) (slice <=
// CEM_SLICE) and selects its min(E, finite) best by a radix select (cem_select: 8-bit digits, LDS histograms with integer
// atomics, stopping as soon as the threshold digit's bin is taken whole; an exact tie at the 64-bit threshold is cut by index).
// With one workgroup (K <= CEM_SLICE) that is the global selection.  Otherwise wave 0 stores the list (index order) and the
// finite count write-through to slab row b, drains and takes an agent-scope ticket; the last workgroup runs the same select
// over the G lists (every global elite is in its own workgroup's list).  That workgroup then ranks the E' elites by counting
// (rank i = #{key_j < key_i} + #{j < i : key_j == key_i}, the list being in index order), and sums the elite rows of U in rank
// order: row-lane r takes ranks r, r + R, ... and the R row-lanes are added in order, once for the mean and once for the
// squared deviations.  Every sum has a fixed order and no float atomics are used: the result is bitwise reproducible.
constexpr int CEM_NT = 256;                 // threads of the update kernel (one histogram bin per thread)
constexpr int CEM_SLICE = 4096;             // candidates per workgroup at most
constexpr int CEM_MAX_ELITE = 1024;
constexpr int CEM_MAX_COLS = 1024;          // 3 N
constexpr unsigned long long CEM_NONE = ~0ull;

struct CemUpdateArgs {
    const void *J, *U;                  // T [K], T [K][3N]
    long long K, slice;                 // candidates, candidates per workgroup
    int C3, G, E, Lcap;                 // 3 N, workgroups, n_elite, slab entries per workgroup (min(CEM_MAX_ELITE, slice))
    double alpha, std[3], std_min[3], lo[3], hi[3];
    const double *mu_in, *sigma_in;     // [3N]; null sigma_in: std[c] on every node
    double *mu_out, *sigma_out;         // [3N]; with shift != 0 mu_out gets the kept mean mu*[min(n + 1, N - 1)]
    int shift;
    long long *elite;                   // [E] rank order, -1 padded, or null
    double *stats;                      // [4] (J rank 0, J rank E'-1, |F|, J_0) or null
    unsigned long long *slab;           // [G][2 + 2 Lcap]: count, finite count, keys, indices (G > 1 only)
    unsigned *ticket;                   // 0 between launches (the last workgroup re-arms it)
    // last iteration of a control step (null record: none): u of the device record <- clamp(mu*[0]); then host_out (mapped)
    // = [record (R), mu* (3N), sigma* (3N), stats (4)], host_elite (mapped) = the elite list, and done_seq released into
    // *done_flag at system scope
    double *record;
    int R;
    double *host_out;
    long long *host_elite;
    unsigned long long *done_flag, done_seq;
    // a step of a device loop (see PlanHandoff): loop.row = [record (R), mu* (3N), sigma* (3N), stats (4), elite list (E, as
    // int64)]; only the loop's last step has a mailbox (host_out, host_elite and done_flag null otherwise)
    PlanHandoff loop;
};

struct CemShared {
    unsigned long long key[CEM_MAX_ELITE];          // the selection in index order
    int idx[CEM_MAX_ELITE];
    int ridx[CEM_MAX_ELITE];                        // ... and its indices in rank order
    unsigned hist[256];
    unsigned wsum[CEM_NT / 64];
    unsigned sel[3];                                // bin, count before it, count in it
    double part[CEM_MAX_COLS];                      // row-lane partial sums
    double mu[CEM_MAX_COLS], sg[CEM_MAX_COLS];
};

RV_DEV unsigned long long cem_key(double v) {      // order-preserving; CEM_NONE (above every finite key) for NaN and +-inf
    if (!::isfinite(v)) return CEM_NONE;
    if (v == 0.0) v = 0.0;                          // -0 ranks with +0
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

// exclusive prefix of v over the workgroup's threads in thread order; total = the sum over the workgroup
RV_DEV unsigned cem_block_scan(unsigned v, unsigned *sW, unsigned &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) sW[wv] = x;
    __syncthreads();
    unsigned off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < CEM_NT / 64; ++w) {
        const unsigned t = sW[w];
        if (w < wv) off += t;
        total += t;
    }
    __syncthreads();
    return off + x - v;
}

// f(i) for i = 0 .. n - 1: unrolled over CAP (> 0) so that f may index a register array by i, or a plain loop (CAP = 0)
template <int CAP, class F>
RV_DEV void cem_for(long long n, const F &f) {
    if constexpr (CAP > 0) {
#pragma unroll
        for (int i = 0; i < CAP; ++i)
            if (i < n) f(i);
    } else {
        for (long long i = 0; i < n; ++i) f(i);
    }
}

// The min(E, n) smallest pairs (key, idx) among positions [0, M) of a source (positions in ascending idx order), into s.key /
// s.idx in index order.  Thread t owns positions [t C, t C + C), C = ceil(M / CEM_NT), and ld(i, key, idx) gives its i-th
// (key CEM_NONE: no candidate); CAP as for cem_for.  Returns their count; n = the candidates' count.
template <int CAP, class Ld>
RV_DEV int cem_select(const Ld &ld, long long M, int E, CemShared &s, unsigned &n) {
    const int tid = threadIdx.x;
    const long long C = (M + CEM_NT - 1) / CEM_NT, p0 = tid * C, mine = p0 >= M ? 0 : (p0 + C < M ? C : M - p0);
    int shift = 64;                     // candidates "equal" so far: those whose bits above `shift` are P
    unsigned long long P = 0;
    unsigned need = 0, cnt = 0;         // elites still to take among the equal ones, and their count
    bool first = true;
    for (;;) {
        s.hist[tid] = 0;
        __syncthreads();
        cem_for<CAP>(mine, [&](auto i) {
            unsigned long long key; int idx;
            ld(i, key, idx);
            if (key != CEM_NONE && (shift == 64 || (key >> shift) == P)) atomicAdd(&s.hist[(key >> (shift - 8)) & 255], 1u);
        });
        __syncthreads();
        const unsigned h = s.hist[tid];
        unsigned tot;
        const unsigned before = cem_block_scan(h, s.wsum, tot);
        if (first) {
            first = false;
            n = tot; cnt = tot; need = tot < (unsigned)E ? tot : (unsigned)E;
            if (need == cnt) break;     // every candidate is an elite (or there is none)
        }
        if (before < need && need <= before + h) { s.sel[0] = tid; s.sel[1] = before; s.sel[2] = h; }
        __syncthreads();
        P = (P << 8) | s.sel[0];
        shift -= 8;
        need -= s.sel[1];
        cnt = s.sel[2];
        if (cnt == need || shift == 0) break;
    }
    // elites: the candidates above P, and of those equal to P all (cnt == need) or the first `need` by index.  Each thread
    // walks its positions twice: counts, one scan, then the writes at their index-order slots.
    const unsigned cap = cnt == need ? 0xffffffffu : need;
    unsigned nlt = 0, neq = 0;
    cem_for<CAP>(mine, [&](auto i) {
        unsigned long long key; int idx;
        ld(i, key, idx);
        const unsigned long long hi = shift == 64 ? 0 : key >> shift;
        nlt += key != CEM_NONE && hi < P;
        neq += key != CEM_NONE && hi == P;
    });
    unsigned tlt, teq;
    unsigned lt = cem_block_scan(nlt, s.wsum, tlt), eq = cem_block_scan(neq, s.wsum, teq);
    cem_for<CAP>(mine, [&](auto i) {
        unsigned long long key; int idx;
        ld(i, key, idx);
        if (key == CEM_NONE) return;
        const unsigned long long hi = shift == 64 ? 0 : key >> shift;
        if (hi < P || (hi == P && eq < cap)) {
            const unsigned at = lt + (eq < cap ? eq : cap);          // < min(E, n) by the counts above
            if (at < CEM_MAX_ELITE) { s.key[at] = key; s.idx[at] = idx; }
        }
        lt += hi < P;
        eq += hi == P;
    });
    __syncthreads();
    return (int)(tlt + (teq < cap ? teq : cap));
}

// The selection and refit of one problem by the workgroups blockIdx.x = 0 .. G - 1 (the kernels below: one problem, or
// blockIdx.y = problem).  QC = columns per thread: 1 when 3 N <= CEM_NT, else 4
template <typename T, int QC>
RV_DEV void cem_update_body(const CemUpdateArgs &a, const PlanBatchAt &at) {
    __shared__ CemShared s;
    __shared__ int sLast;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const T *__restrict__ J = static_cast<const T *>(a.J) + at.b * a.K;
    const T *__restrict__ U = static_cast<const T *>(a.U) + at.b * a.K * a.C3;
    const int C3 = a.C3, G = a.G;
    // the problem's other arrays, each taken from the arguments where it is used
    auto mu_in = [&] { return a.mu_in + at.b * C3; };
    auto sigma_in = [&] { return a.sigma_in + at.b * C3; };            // (a.sigma_in not null)
    auto mu_out = [&] { return a.mu_out + at.b * C3; };
    auto sigma_out = [&] { return a.sigma_out + at.b * C3; };
    auto slab_p = [&] { return a.slab + at.b * at.slab_stride; };      // (G > 1)
    auto ticket = [&] { return a.ticket + at.b; };
    const long long k0 = (long long)blockIdx.x * a.slice, k1 = k0 + a.slice < a.K ? k0 + a.slice : a.K;

    // (1) the workgroup's own selection, its keys in registers (thread t: candidates k0 + t C1 + i, all loads issued at once)
    constexpr int CAP1 = CEM_SLICE / CEM_NT;
    const long long M1 = k1 - k0, C1 = (M1 + CEM_NT - 1) / CEM_NT, q0 = k0 + tid * C1;
    unsigned long long kr[CAP1];
#pragma unroll
    for (int i = 0; i < CAP1; ++i) kr[i] = i < C1 && q0 + i < k1 ? cem_key((double)J[q0 + i]) : CEM_NONE;
    unsigned nfin;
    int nE = cem_select<CAP1>([&](int i, unsigned long long &key, int &idx) {
                                  key = kr[i];
                                  idx = (int)(q0 + i);
                              }, M1, a.E, s, nfin);

    if (G > 1) {
        // (2) wave 0 stores the list write-through to the slab, drains and takes the ticket; the last workgroup selects
        //     again over all the lists
        const long long W = 2 + 2 * (long long)a.Lcap;
        if (wv == 0) {
            unsigned long long *row = slab_p() + blockIdx.x * W;
            for (int i = lane; i < nE; i += 64) {
                st_agent(row + 2 + i, s.key[i]);
                st_agent(row + 2 + a.Lcap + i, (unsigned long long)s.idx[i]);
            }
            if (lane == 0) { st_agent(row, (unsigned long long)nE); st_agent(row + 1, (unsigned long long)nfin); }
            // write-through stores acknowledged before the ticket that announces them (no L2 write-back fence needed)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) sLast = __hip_atomic_fetch_add(ticket(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(G - 1);
        }
        __syncthreads();
        if (!sLast) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: keeps the slab loads below the ticket)
        if (tid == 0) __hip_atomic_store(ticket(), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // |F| = the sum of the workgroups' finite counts
        unsigned f = 0;
        for (int b = tid; b < G; b += CEM_NT) f += (unsigned)ld_agent(slab_p() + b * W + 1);
        cem_block_scan(f, s.wsum, nfin);
        const int Lcap = a.Lcap;
        unsigned ncand;
        const long long C2 = ((long long)G * Lcap + CEM_NT - 1) / CEM_NT;
        nE = cem_select<0>([&](long long i, unsigned long long &key, int &idx) {
                            const long long p = tid * C2 + i, b = p / Lcap;
                            const int j = (int)(p - b * Lcap);
                            const unsigned long long *row = slab_p() + b * W;
                            key = CEM_NONE;
                            if ((unsigned long long)j < ld_agent(row)) {
                                key = ld_agent(row + 2 + j);
                                idx = (int)ld_agent(row + 2 + Lcap + j);
                            }
                        }, (long long)G * Lcap, a.E, s, ncand);
    }

    // (3) rank order
    for (int i = tid; i < nE; i += CEM_NT) {
        const unsigned long long ki = s.key[i];
        int r = 0;
#pragma unroll 8
        for (int j = 0; j < nE; ++j) {
            const unsigned long long kj = s.key[j];
            r += kj < ki || (kj == ki && j < i);
        }
        s.ridx[r] = s.idx[i];
    }
    __syncthreads();

    // (4) mean and spread of the elite rows, in double; threads map to columns, R row-lanes side by side when 3N <= 256
    const int R = C3 <= CEM_NT ? CEM_NT / C3 : 1;
    const int r = C3 <= CEM_NT ? tid / C3 : 0, c0 = C3 <= CEM_NT ? tid - r * C3 : tid;
    const bool active = r < R;
    constexpr int CH = QC == 1 ? 16 : 8;            // elite rows per row-lane whose loads are issued together
    for (int pass = 0; pass < 2 && nE > 0; ++pass) {
        double S[QC];
        double m[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            S[q] = 0.0;
            const int c = c0 + q * CEM_NT;
            m[q] = pass && c < C3 ? s.mu[c] : 0.0;
        }
        if (active) {
            for (int jb = r; jb < nE; jb += CH * R) {
                double uv[CH][QC];
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    const int j = jb + t * R;
                    const long long k = j < nE ? s.ridx[j] : 0;
#pragma unroll
                    for (int q = 0; q < QC; ++q) {
                        const int c = c0 + q * CEM_NT;
                        uv[t][q] = (j < nE && c < C3) ? (double)U[k * C3 + c] : 0.0;
                    }
                }
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    if (jb + t * R >= nE) break;
#pragma unroll
                    for (int q = 0; q < QC; ++q) {
                        const double d = uv[t][q] - m[q];
                        S[q] = pass ? ::fma(d, d, S[q]) : S[q] + uv[t][q];
                    }
                }
            }
        }
        if (C3 <= CEM_NT) {
            if (active) s.part[r * C3 + c0] = S[0];
        } else {
#pragma unroll
            for (int q = 0; q < QC; ++q)
                if (c0 + q * CEM_NT < C3) s.part[c0 + q * CEM_NT] = S[q];
        }
        __syncthreads();
        for (int c = tid; c < C3; c += CEM_NT) {
            double t = s.part[c];
            for (int q = 1; q < R; ++q) t += s.part[q * C3 + c];
            if (pass == 0) s.mu[c] = t / nE;         // m, read by every thread in the second pass
            else s.sg[c] = t / nE;                   // v
        }
        __syncthreads();
    }
    for (int c = tid; c < C3; c += CEM_NT) {
        const int ch = c % 3;
        const double mi = mu_in()[c], si = a.sigma_in ? sigma_in()[c] : a.std[ch];
        if (nE == 0) {
            s.mu[c] = mi; s.sg[c] = si;             // no finite cost: mean and spread stay, bit for bit
        } else {
            s.mu[c] = a.alpha * mi + (1.0 - a.alpha) * s.mu[c];
            s.sg[c] = ::fmax(a.std_min[ch], a.alpha * si + (1.0 - a.alpha) * ::sqrt(s.sg[c]));
        }
    }
    __syncthreads();
    for (int c = tid; c < C3; c += CEM_NT) {
        mu_out()[c] = s.mu[a.shift && c + 3 < C3 ? c + 3 : c];
        sigma_out()[c] = s.sg[c];
    }
    const double nan = __builtin_nan("");
    const double st0 = nE ? (double)J[s.ridx[0]] : nan, st1 = nE ? (double)J[s.ridx[nE - 1]] : nan;
    const double st2 = (double)nfin, st3 = (double)J[0];
    if (a.elite)
        for (int i = tid; i < a.E; i += CEM_NT) a.elite[i] = i < nE ? s.ridx[i] : -1;
    if (a.stats && tid == 0) { a.stats[0] = st0; a.stats[1] = st1; a.stats[2] = st2; a.stats[3] = st3; }
    if (a.record && wv == 0) {
        // the control to apply is clamp(mu*[0]); the rest of the record is the last rollout's
        auto u = [&](int c) { return cem_clamp(s.mu[c], a.lo[c], a.hi[c]); };
        double *record = a.record + at.b * a.R;
        if (lane < 3) record[2 + lane] = u(lane);
        auto row_to = [&](double *o, long long *elite) {
            for (int i = lane; i < a.R; i += 64) o[i] = (i >= 2 && i < 5) ? u(i - 2) : record[i];
            for (int c = lane; c < C3; c += 64) { o[a.R + c] = s.mu[c]; o[a.R + C3 + c] = s.sg[c]; }
            for (int i = lane; i < a.E; i += 64) elite[i] = i < nE ? s.ridx[i] : -1;
            if (lane == 0) { o[a.R + 2 * C3] = st0; o[a.R + 2 * C3 + 1] = st1; o[a.R + 2 * C3 + 2] = st2; o[a.R + 2 * C3 + 3] = st3; }
        };
        if (a.loop.row) {
            double *o = a.loop.row + at.b * a.loop.row_stride;
            row_to(o, reinterpret_cast<long long *>(o + a.R + 2 * C3 + 4));
            plan_handoff_state(a.loop, at.b, record);
        }
        if (a.host_out) {
            row_to(a.host_out + at.b * at.host_stride, a.host_elite + at.b * at.host_stride);
            plan_publish(a.done_flag, a.done_seq, at.step_ticket, at.B);          // (see mppi_update_body)
        }
    }
}

template <typename T, int QC>
__global__ void __launch_bounds__(CEM_NT)
cem_update_kernel(const CemUpdateArgs a) {
    cem_update_body<T, QC>(a, PlanBatchAt{});
}

// Batched form: grid (G, B).  Problem b = blockIdx.y has its own J, U, mean and spread halves, slab rows, ticket, record and
// mailbox row (the elite list inside it), each at the first problem's pointer + b * its stride (PlanBatchAt); within a problem
// everything is cem_update_body, the cross-workgroup select at K > CEM_SLICE included.
struct CemUpdateBatchArgs {
    CemUpdateArgs a;                    // problem 0
    size_t slab_stride, host_stride;    // 64-bit words per problem
    unsigned *step_ticket;              // last iteration: 0 between steps
    int B;
};

template <typename T, int QC>
__global__ void __launch_bounds__(CEM_NT)
cem_update_batch_kernel(const CemUpdateBatchArgs ba) {
    cem_update_body<T, QC>(ba.a, PlanBatchAt{blockIdx.y, ba.slab_stride, ba.host_stride, ba.step_ticket, ba.B});
}

}  // namespace rovmpc
