// discover_kernels.h -- rovmpc_discover_rows: the Gram matrix of M library terms and the target over the recordings of a
// group, then forward orthogonal least squares on it (fp64, gfx950).  The law is in include/rovmpc.h.  Two launches: one
// workgroup per chunk of ROVMPC_DISCOVER_CHUNK rows writes one partial Gram; one wave per group adds the partials in the
// law's order and selects.  No atomics, nothing between workgroups.
#pragma once
#include "util_kernels.h"

namespace rovmpc {

constexpr int DISC_NT = 128;                                  // lanes of a Gram workgroup: two waves
constexpr int DISC_TILE = 64;                                 // rows staged per pass: lane & 63 = the row, lane >> 6 = which terms
constexpr int DISC_LD = DISC_TILE + 1;                        // a column's stride in LDS (odd: columns k, k + 1, ... on distinct banks)
constexpr int DISC_MAXC = ROVMPC_DISCOVER_MAX_TERMS + 1;      // columns: the terms and the target
constexpr int DISC_MAXE = DISC_MAXC * (DISC_MAXC + 1) / 2;    // packed lower triangle
constexpr int DISC_ACC = (DISC_MAXE + DISC_NT - 1) / DISC_NT; // entries a lane accumulates (17)
constexpr int DISC_WAVE = 64;                                 // the selection's workgroup: lane j = term j
static_assert(ROVMPC_DISCOVER_MAX_TERMS <= DISC_WAVE, "one lane per term");
static_assert(ROVMPC_DISCOVER_CHUNK % DISC_TILE == 0, "a chunk is whole tiles but for its last");

struct DiscoverArgs {
    const int32_t *code, *code_off;              // [code_off[M]], [M + 1]
    const double *consts;                        // [const_off[M]]
    const int32_t *const_off;                    // [M + 1]
    const double *X, *target;                    // [B][T][F], [B][T]
    const long long *len;                        // [B] or null
    const long long *chunk_rec, *chunk_row;      // [n_chunks]: the chunk's recording and its first row there
    const long long *group_chunk;                // [G + 1]: the chunks of group g
    const long long *group_n;                    // [G]: its counted rows
    double *partial;                             // [n_chunks][E], E = (M + 1)(M + 2) / 2
    int32_t *picks;                              // [G][S]
    double *coef, *loss, *gram;                  // [G][S][S], [G][S + 1], [G][E] or null
    long long *info;                             // [G][3]
    long long T;
    double dep_tol, min_gain;
    int F, M, S;
};

inline size_t discover_gram_lds_bytes(int M) {
    return ((size_t)ROVMPC_MAX_STACK * DISC_NT + (size_t)(M + 1) * DISC_LD) * sizeof(double);
}

// entry e of the packed lower triangle -> (j, k), k <= j, e = j (j + 1) / 2 + k
RV_DEV void discover_unpack(int e, int &j, int &k) {
    int r = (int)((__builtin_sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while ((r + 1) * (r + 2) / 2 <= e) ++r;
    while (r * (r + 1) / 2 > e) --r;
    j = r; k = e - r * (r + 1) / 2;
}

// Stage 1.  P[j][k] of one chunk: one fused multiply-add per row in increasing row order from +0.
__global__ void __launch_bounds__(DISC_NT)
discover_gram_kernel(const DiscoverArgs a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x, row = lane & (DISC_TILE - 1), half = lane / DISC_TILE;
    double *const lds = reinterpret_cast<double *>(smem_raw);
    double *const stack = lds + lane;                                   // [ROVMPC_MAX_STACK][lane]
    double *const col = lds + (size_t)ROVMPC_MAX_STACK * DISC_NT;       // [M + 1][DISC_LD]
    const int M = a.M, F = a.F, E = (M + 1) * (M + 2) / 2;
    const long long c = blockIdx.x, b = a.chunk_rec[c], r0 = a.chunk_row[c];
    const long long n = a.len ? a.len[b] : a.T;
    const int cnt = (int)(n - r0 < ROVMPC_DISCOVER_CHUNK ? n - r0 : ROVMPC_DISCOVER_CHUNK);
    const double *X = a.X + (size_t)b * a.T * F, *target = a.target + (size_t)b * a.T;

    // the lane's entries e = lane, lane + NT, ...: their two columns, packed; an entry past E reads column 0 and is not written
    int jk[DISC_ACC];
    double acc[DISC_ACC];
#pragma unroll
    for (int q = 0; q < DISC_ACC; ++q) {
        const int e = lane + q * DISC_NT;
        int j = 0, k = 0;
        if (e < E) discover_unpack(e, j, k);
        jk[q] = (j * DISC_LD) << 16 | (k * DISC_LD);
        acc[q] = 0.0;
    }

    for (int t0 = 0; t0 < cnt; t0 += DISC_TILE) {
        const int rows = cnt - t0 < DISC_TILE ? cnt - t0 : DISC_TILE;
        const long long i = r0 + t0 + (row < rows ? row : rows - 1);   // rows past the tile's end repeat its last: uniform control flow
        const double *x = X + i * F;
        for (int t = half; t < M; t += DISC_NT / DISC_TILE) {           // (the program is uniform over the wave)
            const int c0 = a.code_off[t];
            col[t * DISC_LD + row] = interp_eval<double>(a.code + c0, a.code_off[t + 1] - c0, a.consts + a.const_off[t], x, 1, stack, DISC_NT);
        }
        if (half == 0) col[M * DISC_LD + row] = target[i];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
#pragma unroll
            for (int q = 0; q < DISC_ACC; ++q)
                acc[q] = ::fma(col[(jk[q] >> 16) + r], col[(jk[q] & 0xffff) + r], acc[q]);
        }
        __syncthreads();
    }
    double *P = a.partial + (size_t)c * E;
#pragma unroll
    for (int q = 0; q < DISC_ACC; ++q) {
        const int e = lane + q * DISC_NT;
        if (e < E) P[e] = acc[q];
    }
}

// Stage 2.  The group's Gram from its chunk partials, then the forward selection, every operation rounded on its own.
__global__ void __launch_bounds__(DISC_WAVE)
discover_select_kernel(const DiscoverArgs a) {
#pragma clang fp contract(off)
    constexpr int S_MAX = ROVMPC_DISCOVER_MAX_SIZE;
    __shared__ double sG[DISC_MAXE];                  // the packed lower triangle, column M the target
    __shared__ double sW[S_MAX][DISC_WAVE];           // w_j[t]
    __shared__ double sGain[DISC_WAVE], sQ[DISC_WAVE], sRho[DISC_WAVE];
    __shared__ int sCand[DISC_WAVE];
    __shared__ double sZ[S_MAX], sA[S_MAX];
    __shared__ int sPick[S_MAX];
    const int lane = threadIdx.x, M = a.M, S = a.S, E = (M + 1) * (M + 2) / 2;
    const long long g = blockIdx.x, c0 = a.group_chunk[g], c1 = a.group_chunk[g + 1];
    const double nan = m_nan<double>();
    auto G = [&](int j, int k) { return j >= k ? sG[j * (j + 1) / 2 + k] : sG[k * (k + 1) / 2 + j]; };

    for (int e = lane; e < E; e += DISC_WAVE) {
        double s = 0.0;
        for (long long c = c0; c < c1; ++c) s = s + a.partial[(size_t)c * E + e];
        sG[e] = s;
        if (a.gram) a.gram[(size_t)g * E + e] = s;
    }
    __syncthreads();

    int32_t *picks = a.picks + (size_t)g * S;
    double *coef = a.coef + (size_t)g * S * S, *loss = a.loss + (size_t)g * (S + 1);
    for (int e = lane; e < S; e += DISC_WAVE) picks[e] = -1;
    for (int e = lane; e < S * S; e += DISC_WAVE) coef[e] = 0.0;
    for (int e = lane; e <= S; e += DISC_WAVE) loss[e] = nan;

    const double cc = G(M, M), dn = (double)a.group_n[g];
    const bool in = lane < M;
    const double gjj = in ? G(lane, lane) : 0.0, bj = in ? G(M, lane) : 0.0;
    const bool admissible = in && gjj > 0.0 && m_finite(gjj) && m_finite(bj);
    double rho = gjj, qj = bj, Fs = cc;
    bool picked = false;
    int n_sel = 0, status = ROVMPC_DISCOVER_FULL;
    if (!m_finite(cc)) status = ROVMPC_DISCOVER_NONFINITE;
    if (lane == 0) loss[0] = cc / dn;

    for (int s = 0; s < S && status == ROVMPC_DISCOVER_FULL; ++s) {
        const bool cand = admissible && !picked && rho > a.dep_tol * gjj;
        const double gain = (qj * qj) / rho;
        sGain[lane] = gain; sCand[lane] = cand && gain == gain; sQ[lane] = qj; sRho[lane] = rho;
        __syncthreads();
        int p = -1;
        double best = 0.0;
        for (int j = 0; j < M; ++j)
            if (sCand[j] && (p < 0 || sGain[j] > best)) { p = j; best = sGain[j]; }
        if (p < 0) { status = ROVMPC_DISCOVER_EXHAUSTED; break; }
        if (best <= a.min_gain * cc) { status = ROVMPC_DISCOVER_MIN_GAIN; break; }
        const double l = m_sqrt(sRho[p]), z = sQ[p] / l;
        // w_j[s] for every admissible unpicked j; w_p[s] = l
        double w = 0.0;
        if (admissible && !picked) {
            double sum = 0.0;
            for (int t = 0; t < s; ++t) sum = sum + sW[t][p] * sW[t][lane];
            w = lane == p ? l : (G(p, lane) - sum) / l;
            if (lane != p) { rho = rho - w * w; qj = qj - w * z; }
        }
        __syncthreads();                                                // (all reads of sW[.][p] and the scan are done)
        sW[s][lane] = w;
        if (lane == p) picked = true;
        Fs = Fs - z * z;
        if (lane == 0) {
            sZ[s] = z; sPick[s] = p;
            picks[s] = p;
            loss[s + 1] = (Fs > 0.0 ? Fs : 0.0) / dn;
        }
        __syncthreads();
        // the size-(s + 1) row: L^T a = z by back substitution, L's row i the w of pick i
        if (lane == 0) {
            for (int i = s; i >= 0; --i) {
                double sum = 0.0;
                for (int m = i + 1; m <= s; ++m) sum = sum + sW[i][sPick[m]] * sA[m];
                sA[i] = (sZ[i] - sum) / sW[i][sPick[i]];
            }
            for (int i = 0; i <= s; ++i) coef[s * S + i] = sA[i];
        }
        n_sel = s + 1;
        __syncthreads();
    }
    if (lane == 0) {
        long long *info = a.info + (size_t)g * 3;
        info[0] = n_sel; info[1] = status; info[2] = a.group_n[g];
    }
}

}  // namespace rovmpc
