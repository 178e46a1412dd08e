// rovmpc.hip -- C ABI (include/rovmpc.h) over the HIP kernels.  gfx950 only, no torch types.
#include "rovmpc_internal.h"

#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <chrono>
#include <map>

#include "mppi_kernels.h"
#include "cem_kernels.h"
#include "proposal_kernels.h"
#include "nav_kernels.h"
#include "tether_kernels.h"
#include "comm_kernels.h"
#include "embedded_sources.inc"

thread_local std::string g_create_error;

extern "C" const char *rovmpc_version(void) { return "rovmpc 0.1 (gfx950)"; }

extern "C" void rovmpc_default_config(rovmpc_config *c) {
    memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(rovmpc_config);
    c->device = 0; c->dtype = ROVMPC_F64; c->N = 20; c->K = 4096; c->n_shape_pts = 16;
    c->vt_mode = ROVMPC_VT_COMPOSE; c->prev_mode = ROVMPC_PREV_INTERP; c->integrator = ROVMPC_RK4;
    c->frame = ROVMPC_ENU; c->force_interpreter = 0; c->candidates_per_block = 0;
    c->dt = 1.0 / 60.0; c->v_scale = 1e-3; c->L = 3.0; c->cable_wet_weight = 1.521;
    c->c_lo = 1e-6; c->c_hi = 10.0;
    c->w_theta = 1.0; c->w_gamma = 1.0; c->w_u = 1e-6; c->w_T = 1e-2; c->w_taut = 1e3;
    c->rho_taut = 0.98; c->w_floor = 10.0; c->z_floor = -1.2;
}

extern "C" const char *rovmpc_last_error(const rovmpc_handle *h) {
    return h ? h->err.c_str() : g_create_error.c_str();
}

extern "C" int32_t rovmpc_result_len(const rovmpc_handle *h) { return h ? 5 + 2 * (h->cfg.N + 1) : 0; }

// ---- allocation shared by the sampled step, MPPI and CEM: all or nothing, so a call repeated after a failure leaks nothing ----
template <typename P> static void dev_free(P *&p) { if (p) (void)hipFree(p); p = nullptr; }

static void mailbox_free(Mailbox &m) {
    for (void *p : {(void *)m.h_out, (void *)m.h_done}) if (p) (void)hipHostFree(p);
    m = Mailbox();
}

static int mailbox_alloc(rovmpc_handle *h, Mailbox &m, size_t n_doubles) {
    hipError_t e = hipHostMalloc((void **)&m.h_out, n_doubles * sizeof(double), hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&m.d_out, m.h_out, 0);
    if (e == hipSuccess) e = hipHostMalloc((void **)&m.h_done, 64, hipHostMallocMapped);
    if (e == hipSuccess) { *m.h_done = 0; e = hipHostGetDevicePointer((void **)&m.d_done, m.h_done, 0); }
    if (e == hipSuccess) return ROVMPC_OK;
    mailbox_free(m);
    FAIL(h, ROVMPC_ERR_HIP, "mapped host memory for a step's results: %s", hipGetErrorString(e));
}

static void slab_free(Slab &s) { dev_free(s.rows); dev_free(s.ticket); }

// bytes = 0: an update of one workgroup needs the ticket only.  Nothing to do when the slab is there.
static int slab_alloc(rovmpc_handle *h, Slab &s, size_t bytes) {
    if (s.ticket) return ROVMPC_OK;
    hipError_t e = bytes ? hipMalloc(&s.rows, bytes) : hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&s.ticket, 16);
    if (e == hipSuccess) e = hipMemset(s.ticket, 0, 16);
    if (e == hipSuccess) return ROVMPC_OK;
    slab_free(s);
    FAIL(h, ROVMPC_ERR_HIP, "update slab: %s", hipGetErrorString(e));
}

static void plan_free(PlanCtl &c) {
    dev_free(c.U); dev_free(c.J); dev_free(c.state); dev_free(c.record); dev_free(c.seeds); dev_free(c.plan); dev_free(c.spread);
    dev_free(c.slab); dev_free(c.tickets);
    if (c.h_stage) (void)hipHostFree(c.h_stage);
    c.h_stage = c.d_stage = nullptr;
    mailbox_free(c.box);
    c.B = 0;
}

// Into a fresh PlanCtl, all or nothing: the caller swaps it in, so a failure leaves the previous state usable.  The
// controller's sizes: 64-bit words of a problem's slab and of its mailbox row, a spread next to the plan.
static int plan_alloc(rovmpc_handle *h, PlanCtl &c, int B, size_t slab_words, size_t row_words, bool with_spread) {
    const size_t K = (size_t)h->cfg.K, C3 = 3 * (size_t)h->cfg.N, R = (size_t)rovmpc_result_len(h), nb = (size_t)B;
    hipError_t e = hipSuccess;
    auto dev = [&e](auto **p, size_t bytes) { if (e == hipSuccess) e = hipMalloc((void **)p, bytes); };
    dev(&c.U, nb * K * C3 * h->esz); dev(&c.J, nb * K * h->esz);
    dev(&c.state, nb * ROVMPC_STATE_LEN * sizeof(double)); dev(&c.record, nb * R * sizeof(double));
    if (!c.single) dev(&c.seeds, nb * sizeof(unsigned long long));
    dev(&c.plan, 2 * nb * C3 * sizeof(double));
    if (with_spread) dev(&c.spread, 2 * nb * C3 * sizeof(double));
    if (slab_words) dev(&c.slab, nb * slab_words * 8);
    dev(&c.tickets, (nb + 1) * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(c.tickets, 0, (nb + 1) * sizeof(unsigned));
    if (!c.single) {
        if (e == hipSuccess) e = hipHostMalloc((void **)&c.h_stage, nb * (ROVMPC_STATE_LEN + 1) * 8, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&c.d_stage, c.h_stage, 0);
    }
    int rc = ROVMPC_OK;
    if (e != hipSuccess) { h->err = std::string(c.single ? "" : "batched ") + c.name + " buffers: " + hipGetErrorString(e); rc = ROVMPC_ERR_HIP; }
    if (!rc) rc = mailbox_alloc(h, c.box, nb * row_words);
    if (rc) { plan_free(c); return rc; }
    c.B = B; c.slab_stride = slab_words; c.row = row_words;
    return ROVMPC_OK;
}

static size_t lds_need(const rovmpc_config *c, int ck, int model, unsigned used = 0xffffffffu, int jit_gi = 0) {
    return c->dtype == ROVMPC_F64 ? rollout_lds_elems<double>(c->N, ck, model, c->vt_mode, used, jit_gi) * sizeof(double)
                                  : rollout_lds_elems<float>(c->N, ck, model, c->vt_mode, used, jit_gi) * sizeof(float);
}

static int pick_ck(const rovmpc_config *c, int model, unsigned used, int n_cu, int jit_gi = 0) {
    if (c->candidates_per_block > 0) return c->candidates_per_block;
    // 16 candidates x 4 role lanes fill one wave in the sequential phase of the compiled-in
    // model; shrink only to keep two workgroups per CU inside the 160 KiB of LDS
    int ck = 16;
    // large candidate sets: bigger workgroups (up to 64 candidates = four integrating waves, one
    // per SIMD) keep about one workgroup per CU instead of queueing several rounds of small ones
    while (ck < 64 && c->K / (ck * 2) >= 256) ck *= 2;
    // up to one 16-candidate workgroup per CU a workgroup may take the CU's whole LDS (two workgroups sharing a CU put
    // their integrating waves in each other's way: measured +25 % on the slower of the two); beyond that keep two per CU
    const bool one_per_cu = (c->K + ck - 1) / ck <= n_cu;
    const size_t cap = (ck > 16 || one_per_cu) ? 160 * 1024 : 80 * 1024;
    while (ck > 1 && lds_need(c, ck, model, used, jit_gi) > cap) ck /= 2;
    return ck;
}

// ---- which instance a launch runs: the only place that names the rollout kernels ------------------------------------------
struct Variant { LaunchKind kind; int N, CK; bool lean, literal_n; };       // {LAUNCH_PLAIN, 0, 0, false, false}: the generic kernel

template <typename T, int MODEL, int VT> static const void *rollout_instance(const Variant &v) {
    if constexpr (MODEL == MODEL_INTERP) {
        return v.kind == LAUNCH_PLAIN ? (const void *)rollout_kernel<T, MODEL, VT> : nullptr;      // (one instance of the interpreter kernel)
    } else {
        // the literal-CK instances (see rollout_body, CKC), and with them the literal horizons of the BASELINE configurations
        // (NC: N = 20 in double precision, N = 50 in single)
        const bool ck16 = v.CK == 16, n20 = sizeof(T) == 8 && ck16 && v.N == 20 && v.literal_n;
        if (v.kind == LAUNCH_SAMPLED) return (const void *)rollout_kernel_sampled<T, MODEL, VT>;
        if (v.kind == LAUNCH_STEP) {
            if constexpr (sizeof(T) == 8) { if (n20) return (const void *)closed_loop_step_kernel16_n20<T, MODEL, VT>; }
            return ck16 ? (const void *)closed_loop_step_kernel16<T, MODEL, VT> : (const void *)closed_loop_step_kernel<T, MODEL, VT>;
        }
        if (3 * v.N + 2 > 64) {                                               // long horizons: see rollout_body, LONGH
            if constexpr (sizeof(T) == 4) { if (v.lean && ck16 && v.N == 50 && v.literal_n) return (const void *)rollout_kernel_long_lean16_n50<T, MODEL, VT>; }
            if (v.lean) return ck16 ? (const void *)rollout_kernel_long_lean16<T, MODEL, VT> : (const void *)rollout_kernel_long_lean<T, MODEL, VT>;
            return ck16 ? (const void *)rollout_kernel_long16<T, MODEL, VT> : (const void *)rollout_kernel_long<T, MODEL, VT>;
        }
        if constexpr (sizeof(T) == 8) { if (n20) return v.lean ? (const void *)rollout_kernel_lean16_n20<T, MODEL, VT> : (const void *)rollout_kernel16_n20<T, MODEL, VT>; }
        if (v.lean) return ck16 ? (const void *)rollout_kernel_lean16<T, MODEL, VT> : (const void *)rollout_kernel_lean<T, MODEL, VT>;
        return ck16 ? (const void *)rollout_kernel16<T, MODEL, VT> : (const void *)rollout_kernel<T, MODEL, VT>;
    }
}

template <typename T, int MODEL> static const void *instance_by_vt(int vt, const Variant &v) {
    return vt == 0 ? rollout_instance<T, MODEL, 0>(v) : vt == 1 ? rollout_instance<T, MODEL, 1>(v) : rollout_instance<T, MODEL, 2>(v);
}

// model: MODEL_BUILTIN or MODEL_INTERP (the hiprtc module brings its own two functions)
static const void *compiled_instance(const rovmpc_config &c, int model, const Variant &v) {
    if (c.dtype == ROVMPC_F64) return model == MODEL_BUILTIN ? instance_by_vt<double, MODEL_BUILTIN>(c.vt_mode, v) : instance_by_vt<double, MODEL_INTERP>(c.vt_mode, v);
    return model == MODEL_BUILTIN ? instance_by_vt<float, MODEL_BUILTIN>(c.vt_mode, v) : instance_by_vt<float, MODEL_INTERP>(c.vt_mode, v);
}

// Registers per lane of the compiled-in kernel for this handle's (dtype, vt_mode), from the code object.
static int builtin_kernel_regs(const rovmpc_handle *h) {
    const void *f = compiled_instance(h->cfg, MODEL_BUILTIN, {LAUNCH_PLAIN, 0, 0, false, false});
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, f) != hipSuccess || fa.numRegs <= 0) return 128;
    return fa.numRegs;
}

// Throughput geometry of the compiled-in model when the candidate set is more than one 16-candidate
// workgroup per CU.  A workgroup alone on a CU spends most of its life in the sequential theta chain
// (one wave issuing every ~6 cycles), so what matters is how many waves are RESIDENT per CU:
//   wave slots per SIMD  S = 512 / registers per lane (f64: 3, f32: 6);
//   workgroups per CU by slots: w = NT/64 waves each; w <= 4 -> 4S / w, w > 4 -> S / ceil(w / 4)
//     (measured with the HW_ID stamp of the diagnostic build: a 5-wave workgroup of the f64 kernel is
//      alone on its CU, 4-wave ones run three at a time, 3-wave ones four);
//   workgroups per CU by LDS: 160 KiB / bytes per workgroup.
// Choose (CK, NT) maximising resident waves, then resident candidates, then CK (the candidate-
// invariant gamma wave is paid once per workgroup).  CK stays >= 16: fewer leaves theta-wave lanes
// idle.  tools/geometry_sweep.py measures the whole grid; this rule picks its minimum at
// (N 20, f64), (N 20, f32), (N 50, f32) and (N 50, f64) for K = 8192 .. 32768.
static bool throughput_geometry(const rovmpc_handle *h, int n_cu, long long candidates_in_flight, int *ck_out, int *nt_out) {
    const rovmpc_config *c = &h->cfg;
    if ((candidates_in_flight + 15) / 16 <= n_cu) return false;
    int alloc = (builtin_kernel_regs(h) + 7) / 8 * 8;
    int S = 512 / alloc; if (S > 8) S = 8; if (S < 1) S = 1;
    long best_w = -1, best_c = -1; int best_ck = 0, best_nt = 0;
    for (int ck = 16; ck <= 64; ck *= 2) {
        const size_t lds = lds_need(c, ck, MODEL_BUILTIN);
        if (lds > 160 * 1024) break;
        const int by_lds = (int)((160 * 1024) / lds);
        for (int nt = 256; nt <= 512; nt += 128) {
            const int w = nt / 64;
            if (w < ck / 16 + 2) continue;                 // theta waves + gamma wave + one geometry wave
            const int by_slots = w <= 4 ? 4 * S / w : S / ((w + 3) / 4);
            const int R = by_slots < by_lds ? by_slots : by_lds;
            if (R < 1) continue;
            const long W = (long)R * w, Cn = (long)R * ck;
            if (W > best_w || (W == best_w && (Cn > best_c || (Cn == best_c && ck > best_ck)))) {
                best_w = W; best_c = Cn; best_ck = ck; best_nt = nt;
            }
        }
    }
    if (best_ck == 0) return false;
    *ck_out = best_ck; *nt_out = best_nt;
    return true;
}

// Launch geometry for the model variant in use.  The per-block buffers are allocated for the
// worst case (one candidate per workgroup) so re-deciding it at set_model needs no allocation.
// strict = false (rovmpc_create, model not known yet): an explicit candidates_per_block that the
// interpreter's LDS layout cannot hold is not an error until a model that needs it is set.
static const char *configure_geometry(rovmpc_handle *h, int model, bool strict = true) {
    const rovmpc_config *cfg = &h->cfg;
    if (strict) {
        hipDeviceProp_t prop{};
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) h->n_cu = prop.multiProcessorCount;
    }
    h->CK = pick_ck(cfg, model, model == MODEL_JIT ? jit_lds_planes(h->used_planes, cfg->vt_mode, cfg->feature_map) : 0xffffffffu, h->n_cu, h->jit_gi);
    // one thread per (candidate, horizon step) of the workgroup when that fits 512 threads, so
    // the per-node geometry phase is a single round
    int items = cfg->N * h->CK;
    h->NT = items >= 512 ? 512 : ((items + 63) / 64) * 64;
    if (strict && model == MODEL_BUILTIN && cfg->candidates_per_block == 0 && cfg->threads_per_block == 0) {
        int ck = 0, nt = 0;
        if (throughput_geometry(h, h->n_cu, cfg->K, &ck, &nt)) { h->CK = ck; h->NT = nt; }
    }
    h->nblocks = (cfg->K + h->CK - 1) / h->CK;
    if (cfg->threads_per_block > 0) h->NT = cfg->threads_per_block;
    if (h->NT < 64 * ((h->CK + 15) / 16)) h->NT = 64 * ((h->CK + 15) / 16);
    if (strict && lds_need(cfg, h->CK, model, model == MODEL_JIT ? jit_lds_planes(h->used_planes, cfg->vt_mode, cfg->feature_map) : 0xffffffffu, h->jit_gi) > 160 * 1024)
        return "rollout workgroup needs more than 160 KiB of LDS; lower candidates_per_block or N";
    return nullptr;
}


// Geometry of one launch: B problems of K candidates each in the grid (B = 1: the handle's own geometry).
Geo launch_geometry(const rovmpc_handle *h, int B) {
    Geo g{h->CK, h->NT, h->nblocks};
    const rovmpc_config *cfg = &h->cfg;
    if (B > 1 && h->model_kind == MODEL_BUILTIN && cfg->candidates_per_block == 0 && cfg->threads_per_block == 0) {
        // what counts is the number of candidates in the grid, whichever problem they belong to
        int ck = 0, nt = 0;
        if (throughput_geometry(h, h->n_cu, (long long)B * cfg->K, &ck, &nt)) {
            while (ck > 16 && ck > cfg->K) ck /= 2;              // never wider than a problem
            g.CK = ck; g.NT = nt;
            if (g.NT < 64 * ((g.CK + 15) / 16)) g.NT = 64 * ((g.CK + 15) / 16);
            g.nblocks = (cfg->K + g.CK - 1) / g.CK;
        }
    }
    return g;
}

// One high-priority stream per device for the whole process, created (and used once, so that the runtime binds it to a
// hardware queue) by the first rovmpc_create on that device: the second stream of the pipelined closed loop.  Measured: the
// same stream created later -- after other streams of the process have run kernels side by side -- can land on a queue
// that serialises with the caller's (31 us per step instead of 15); created first, it keeps its queue whatever comes after.
static std::mutex g_pipe_mu;
static std::map<int, hipStream_t> g_pipe_stream;
static hipStream_t process_pipe_stream(int device) {
    std::lock_guard<std::mutex> lk(g_pipe_mu);
    auto it = g_pipe_stream.find(device);
    if (it != g_pipe_stream.end()) return it->second;
    hipStream_t st = nullptr;
    int lo = 0, hi = 0;
    void *scratch = nullptr;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi) != hipSuccess) st = nullptr;
    if (st && hipMalloc(&scratch, 256) == hipSuccess) {
        (void)hipMemsetAsync(scratch, 0, 256, st);
        (void)hipStreamSynchronize(st);
        (void)hipFree(scratch);
    }
    g_pipe_stream[device] = st;
    return st;
}

extern "C" int rovmpc_create(const rovmpc_config *cfg, rovmpc_handle **out) {
    rovmpc_handle *nullh = nullptr;
    if (!cfg || !out) FAIL(nullh, ROVMPC_ERR_INVALID, "rovmpc_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(rovmpc_config))
        FAIL(nullh, ROVMPC_ERR_INVALID, "rovmpc_create: struct_size %d != %d (ABI mismatch)", cfg->struct_size,
             (int)sizeof(rovmpc_config));
    if (cfg->N < 1 || cfg->N > 4096) FAIL(nullh, ROVMPC_ERR_INVALID, "N must be in 1..4096 (got %d)", cfg->N);
    if (cfg->K < 1) FAIL(nullh, ROVMPC_ERR_INVALID, "K must be >= 1 (got %d)", cfg->K);
    if (cfg->dtype != ROVMPC_F64 && cfg->dtype != ROVMPC_F32) FAIL(nullh, ROVMPC_ERR_INVALID, "bad dtype %d", cfg->dtype);
    if (cfg->n_shape_pts < 2) FAIL(nullh, ROVMPC_ERR_INVALID, "n_shape_pts must be >= 2");
    if (cfg->vt_mode < 0 || cfg->vt_mode > 2) FAIL(nullh, ROVMPC_ERR_INVALID, "bad vt_mode %d", cfg->vt_mode);
    if (cfg->prev_mode < 0 || cfg->prev_mode > 1) FAIL(nullh, ROVMPC_ERR_INVALID, "bad prev_mode %d", cfg->prev_mode);
    if (cfg->integrator < 0 || cfg->integrator > 1) FAIL(nullh, ROVMPC_ERR_INVALID, "bad integrator %d", cfg->integrator);
    if (cfg->frame < 0 || cfg->frame > 1) FAIL(nullh, ROVMPC_ERR_INVALID, "bad frame %d", cfg->frame);
    if (cfg->feature_map < 0 || cfg->feature_map > 2) FAIL(nullh, ROVMPC_ERR_INVALID, "bad feature_map %d", cfg->feature_map);
    if (!(cfg->dt > 0) || !(cfg->L > 0) || !(cfg->c_lo > 0) || !(cfg->c_hi > cfg->c_lo))
        FAIL(nullh, ROVMPC_ERR_INVALID, "dt, L must be > 0 and 0 < c_lo < c_hi");
    if (cfg->candidates_per_block < 0 || cfg->candidates_per_block > 64 ||
        (cfg->candidates_per_block & (cfg->candidates_per_block - 1)) != 0)
        FAIL(nullh, ROVMPC_ERR_INVALID, "candidates_per_block must be 0 (auto) or a power of two <= 64");
    if (cfg->threads_per_block < 0 || cfg->threads_per_block > 512 || cfg->threads_per_block % 64 != 0)
        FAIL(nullh, ROVMPC_ERR_INVALID, "threads_per_block must be 0 (auto) or a multiple of 64 up to 512");
    if ((long long)cfg->N * 3 * 64 >= 65536) FAIL(nullh, ROVMPC_ERR_INVALID, "N must be below 341 (LDS-resident horizon)");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        FAIL(nullh, ROVMPC_ERR_HIP, "no HIP device available (%s); librovmpc has no CPU fallback",
             e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (cfg->device < 0 || cfg->device >= ndev) FAIL(nullh, ROVMPC_ERR_INVALID, "device %d out of range (0..%d)", cfg->device, ndev - 1);

    rovmpc_handle *h = new rovmpc_handle();
    h->cfg = *cfg;
    h->esz = cfg->dtype == ROVMPC_F64 ? 8 : 4;
    if (const char *why = configure_geometry(h, MODEL_INTERP, false)) {
        g_create_error = why;
        delete h;
        return ROVMPC_ERR_INVALID;
    }
    const int max_blocks = cfg->candidates_per_block > 0 ? h->nblocks : cfg->K;
#define CR(call)                                                                         \
    do {                                                                                 \
        hipError_t _e = (call);                                                          \
        if (_e != hipSuccess) {                                                          \
            char _b[256];                                                                \
            snprintf(_b, sizeof(_b), "%s failed: %s", #call, hipGetErrorString(_e));     \
            g_create_error = _b;                                                         \
            rovmpc_destroy(h);                                                           \
            return ROVMPC_ERR_HIP;                                                       \
        }                                                                                \
    } while (0)
    CR(hipSetDevice(cfg->device));
    CR(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->pipe_streams[1] = process_pipe_stream(cfg->device);
    const size_t R = 5 + 2 * (size_t)(cfg->N + 1);
    CR(hipMalloc(&h->d_U, (size_t)cfg->K * cfg->N * 3 * h->esz));
    CR(hipMalloc(&h->d_J, (size_t)cfg->K * h->esz));
    CR(hipMalloc((void **)&h->d_state, ROVMPC_STATE_LEN * sizeof(double)));
    CR(hipMalloc((void **)&h->d_blk_traj, (size_t)max_blocks * (cfg->N + 1) * 2 * sizeof(double)));
    CR(hipMalloc((void **)&h->d_result, R * sizeof(double)));
    CR(hipHostMalloc((void **)&h->h_result, R * sizeof(double), hipHostMallocDefault));
    CR(hipMalloc((void **)&h->d_code_th, ROVMPC_MAX_CODE * sizeof(int32_t)));
    CR(hipMalloc((void **)&h->d_code_ga, ROVMPC_MAX_CODE * sizeof(int32_t)));
    CR(hipMalloc(&h->d_consts, ROVMPC_MAX_CODE * 8));
    CR(hipMalloc((void **)&h->d_consts64, ROVMPC_MAX_CODE * 8));
    CR(hipMalloc(&h->d_Rtab, (size_t)cfg->N * 9 * h->esz));
    CR(hipMalloc(&h->d_k, sizeof(RolloutConsts<double>)));
    CR(hipMalloc((void **)&h->d_granules, gran_stride((int)max_blocks, cfg->N) * sizeof(unsigned long long)));
    CR(hipMemset(h->d_granules, 0, gran_stride((int)max_blocks, cfg->N) * sizeof(unsigned long long)));
    h->epoch_ctr = new unsigned(0);
    CR(hipMalloc(&h->d_gtab, (size_t)8 * (cfg->N + 1) * 8 + 64));
    CR(hipMemset(h->d_gtab, 0, (size_t)8 * (cfg->N + 1) * 8 + 64));
    CR(hipHostMalloc((void **)&h->h_err, 64, hipHostMallocMapped));
    *h->h_err = 0;
    CR(hipHostGetDevicePointer((void **)&h->d_err, h->h_err, 0));
#ifdef ROVMPC_STAMPS
    CR(hipMalloc((void **)&h->d_stamps, (size_t)max_blocks * RV_NSTAMP * sizeof(unsigned long long)));
    CR(hipMemset(h->d_stamps, 0, (size_t)max_blocks * RV_NSTAMP * sizeof(unsigned long long)));
#endif
#undef CR
    *out = h;
    return ROVMPC_OK;
}

extern "C" void rovmpc_destroy(rovmpc_handle *h) {
    if (!h) return;
    (void)rovmpc_comm_destroy(h);
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto &e : h->ev) (void)hipEventDestroy(e);
    void *ptrs[] = {h->d_U, h->d_J, h->d_traj_all, h->d_state, h->d_blk_traj,
                    h->d_result, h->d_code_th, h->d_code_ga, h->d_consts, h->d_consts64, h->d_Rtab, h->d_k, h->d_stamps,
                    h->d_granules, h->d_gtab, h->d_Jb, h->d_blk_trajb, h->d_granulesb, h->d_step_seq, h->d_Us[0], h->d_Us[1], h->d_cl_granules, h->d_cl_blk_traj, h->d_best, h->d_blk_u,
                    h->d_nav_track, h->d_nav_spheres, h->d_tether_spheres, h->d_tether_traj, h->d_score_prog,
                    h->d_discover_partial};
    for (auto &ev : h->pipe_ev) if (ev) (void)hipEventDestroy(ev);
    if (h->score_prog_ev) (void)hipEventDestroy(h->score_prog_ev);
    calib_free(h);
    if (h->pipe_stream_owned && h->pipe_streams[1]) (void)hipStreamDestroy(h->pipe_streams[1]);
    mailbox_free(h->samp_box);
    if (h->h_err) (void)hipHostFree(h->h_err);
    for (PlanCtl *c : {&h->mppi, &h->cem, &h->mppi_b, &h->cem_b}) plan_free(*c);
    slab_free(h->mppi_slab_x); slab_free(h->cem_slab_x);
    for (void *p : ptrs) if (p) (void)hipFree(p);
    delete h->epoch_ctr;
    if (h->h_result) (void)hipHostFree(h->h_result);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

template <typename T> static void fill_consts(const rovmpc_handle *h, RolloutConsts<T> &k) {
    const rovmpc_config &c = h->cfg;
    k.h = (T)c.dt; k.vs_h = (T)(c.v_scale * c.dt); k.vs = (T)c.v_scale; k.inv_h = (T)(1.0 / c.dt); k.L = (T)c.L;
    k.w_per_len = (T)(c.cable_wet_weight / c.L); k.c_lo = (T)c.c_lo; k.c_hi = (T)c.c_hi;
    k.up = c.frame == ROVMPC_ENU ? (T)1 : (T)-1;
    k.inv_Mm1 = (T)(1.0 / (double)(c.n_shape_pts - 1));
    k.w_theta = (T)c.w_theta; k.w_gamma = (T)c.w_gamma; k.w_u = (T)c.w_u; k.w_T = (T)c.w_T;
    k.w_taut = (T)c.w_taut; k.rhoL = (T)(c.rho_taut * c.L); k.w_floor = (T)c.w_floor; k.z_floor = (T)c.z_floor;
    k.theta_ref = (T)c.theta_ref; k.gamma_ref = (T)c.gamma_ref;
    for (int i = 0; i < 3; ++i) k.Uref[i] = (T)c.U_ref[i];
    for (int i = 0; i < 18; ++i) {
        k.mean[i] = i < h->n_feat ? (T)h->mean[i] : (T)0;
        k.inv_scale[i] = i < h->n_feat ? (T)(1.0 / h->scale[i]) : (T)1;
    }
}

// ---- run-time specialisation (hiprtc) ---------------------------------------------------------
// A loaded model that is not the compiled-in one is translated from its bytecode to two C++
// expressions and the rollout kernel is compiled around them (MODEL_JIT): same kernel source as
// the library (embedded at build time), features in registers, no interpreter.  Only bytecode
// that passed validate_code() reaches this point; no source text crosses the C ABI.

static std::string fmt_const(double v) {
    char b[64];
    if (std::isnan(v)) return "m_nan<T>()";
    if (std::isinf(v)) return v > 0 ? "m_inf<T>()" : "(-m_inf<T>())";
    snprintf(b, sizeof(b), "%.17g", v);
    std::string t = b;
    if (t.find_first_of(".eEn") == std::string::npos) t += ".0";
    return "T(" + t + ")";
}

// C++ text of one expression.  Stage-invariant subexpressions are hoisted: of the 18 slots a stage sees, only the state
// slots (`state_mask`) change between the four RK4 stages of a step; everything else comes from the row of a node (start,
// end) or their midpoint, the end row of one step is the start row of the next, and stages two and three share the
// midpoint.  A maximal subtree without a state slot that holds at least one expensive operation (sin, cos, tanh, exp, log,
// sqrt, pow, a division) is therefore emitted once into `subs` -- evaluated per ROW, twice per step instead of four times --
// and referenced as e[k]; `a / D` with a stage-invariant D becomes a * e[k], e[k] = 1 / D (one more rounding, <= 1.5 ulp).
// Both expressions share the list (identical subtrees get one entry); at most ROVMPC_MAX_SUBS of them, the rest stay inline.
constexpr int ROVMPC_MAX_SUBS = 8;
constexpr int ROVMPC_MAX_GSUBS = 2;         // x17-only subexpressions the gamma wave tabulates (rollout_kernels.h: JIT_GROW)
// gsubs (optional): the same for subtrees of dtheta/dt that read the slots of `gmask` alone (the gamma delay slot x17 when the
// gamma path is candidate-invariant): emitted as g[k], evaluated by the gamma wave once per row and workgroup.
static std::string bytecode_to_cxx(const int32_t *code, int n, const double *consts, unsigned state_mask = 0xffffffffu,
                                   std::vector<std::string> *subs = nullptr, std::vector<std::string> *gsubs = nullptr, unsigned gmask = 0) {
    struct Item { std::string text; unsigned slots; int heavy; bool leaf; };
    std::vector<Item> st;
    auto is_exo = [&](const Item &it) { return (it.slots & state_mask) == 0; };
    auto is_g = [&](const Item &it) { return gsubs && it.slots != 0 && (it.slots & ~gmask) == 0; };
    auto hoist_into = [&](Item &it, std::vector<std::string> *list, const char *name, int cap) {
        int k = -1;
        for (size_t q = 0; q < list->size(); ++q) if ((*list)[q] == it.text) k = (int)q;
        if (k < 0) {
            if ((int)list->size() >= cap) return;
            list->push_back(it.text); k = (int)list->size() - 1;
        }
        it.text = std::string(name) + "[" + std::to_string(k) + "]"; it.heavy = 0; it.leaf = true;
    };
    auto hoist = [&](Item &it) {            // replace a stage-invariant, expensive subtree by e[k] (or g[k])
        if (it.heavy == 0) return;
        if (subs && is_exo(it)) hoist_into(it, subs, "e", ROVMPC_MAX_SUBS);
        else if (is_g(it)) hoist_into(it, gsubs, "g", ROVMPC_MAX_GSUBS);
    };
    // the class of a subtree: 0 = reads a slot outside both sets, 1 = stage-invariant (no state slot), 2 = gamma-delay-slot only
    auto cls = [&](const Item &it) { return is_exo(it) ? 1 : (is_g(it) ? 2 : 0); };
    for (int pc = 0; pc < n; ++pc) {
        const int op = code[pc] & 0xff, arg = code[pc] >> 8;
        auto un = [&](const char *f, int cost) {
            Item &a = st.back();
            a.text = std::string(f) + "(" + a.text + ")"; a.heavy += cost; a.leaf = false;
        };
        auto bin = [&](const char *pre, const char *mid, const char *post, int cost) {
            Item b = st.back(); st.pop_back();
            Item &a = st.back();
            // a side whose class the combination loses ends here: it is maximal (a constant-only side joins either class)
            const bool a_const = a.slots == 0, b_const = b.slots == 0;
            if (!a_const && !b_const && cls(a) != cls(b)) { hoist(a); hoist(b); }
            else if (cls(a) == 0 && b_const && b.heavy) hoist(b);
            else if (cls(b) == 0 && a_const && a.heavy) hoist(a);
            a.text = std::string(pre) + a.text + mid + b.text + post;
            a.slots |= b.slots; a.heavy += b.heavy + cost; a.leaf = false;
        };
        const size_t need = op <= ROVMPC_OP_PUSH_F ? 0 : ((op >= ROVMPC_OP_ADD && op <= ROVMPC_OP_DIV) || op == ROVMPC_OP_POW) ? 2 : 1;
        if (st.size() < need) return "m_nan<T>()";          // (validate_code has already checked the stack discipline)
        switch (op) {
        case ROVMPC_OP_PUSH_C: st.push_back({fmt_const(consts[arg]), 0u, 0, true}); break;
        case ROVMPC_OP_PUSH_F: st.push_back({"x[" + std::to_string(arg) + "]", arg < 32 ? (1u << arg) : 0x80000000u, 0, true}); break;
        case ROVMPC_OP_ADD: bin("(", " + ", ")", 0); break;
        case ROVMPC_OP_SUB: bin("(", " - ", ")", 0); break;
        case ROVMPC_OP_MUL: bin("(", " * ", ")", 0); break;
        case ROVMPC_OP_DIV: {
            Item &b = st.back(), &a = st[st.size() - 2];
            const bool b_const = b.leaf && b.text.compare(0, 2, "T(") == 0;
            if (subs && is_exo(b) && !is_exo(a) && !b_const) {          // a / D, D stage-invariant: a * (1 / D), the reciprocal per row
                Item r = {"m_divx(T(1), " + b.text + ")", b.slots, b.heavy + 1, false};
                hoist(r);
                if (r.leaf) { b = r; bin("(", " * ", ")", 0); break; }
            }
            bin("m_divx(", ", ", ")", 1);
            break;
        }
        case ROVMPC_OP_POW: bin("m_pow(", ", ", ")", 1); break;
        case ROVMPC_OP_NEG: un("-", 0); break;
        case ROVMPC_OP_SIN: un("tg.sin", 1); break;
        case ROVMPC_OP_COS: un("m_cos", 1); break;
        case ROVMPC_OP_TANH: un("m_tanh", 1); break;
        case ROVMPC_OP_ABS: un("m_abs", 0); break;
        case ROVMPC_OP_SQUARE: un("rv_sq", 0); break;
        case ROVMPC_OP_EXP: un("m_exp", 1); break;
        case ROVMPC_OP_LOG: un("m_log", 1); break;
        case ROVMPC_OP_SQRT: un("m_sqrt", 1); break;
        case ROVMPC_OP_POWI: { const int e = arg >= (1 << 23) ? arg - (1 << 24) : arg;
                               Item &a = st.back(); a.text = "rv_powi(" + a.text + ", " + std::to_string(e) + ")"; a.heavy += (e < 0); a.leaf = false; break; }
        case ROVMPC_OP_SAFE_LOG: { Item &a = st.back(); a.text = "m_log(m_abs(" + a.text + ") + T(1e-5))"; a.heavy += 1; a.leaf = false; break; }
        case ROVMPC_OP_SAFE_SQRT: { Item &a = st.back(); a.text = "m_sqrt(m_abs(" + a.text + "))"; a.heavy += 1; a.leaf = false; break; }
        default: return "m_nan<T>()";
        }
    }
    if (st.empty()) return "m_nan<T>()";
    hoist(st.back());                                          // an expression that no stage state enters at all
    return st.back().text;
}

// slots a program reads (bit j = feature j)
static unsigned program_slots(const int32_t *code, int n) {
    unsigned m = 0;
    for (int pc = 0; pc < n; ++pc)
        if ((code[pc] & 0xff) == ROVMPC_OP_PUSH_F && (code[pc] >> 8) < 32) m |= 1u << (code[pc] >> 8);
    return m;
}

struct JitModule { hipModule_t mod = nullptr; hipFunction_t fn = nullptr, fn_step = nullptr; };
static std::mutex g_jit_mu;
static std::map<std::string, JitModule> g_jit_cache;     // key: device ordinal + generated source

// Returns nullptr and fills `why` when hiprtc cannot produce the kernel.
static hipFunction_t jit_build(int device, const std::string &src, std::string &why, hipFunction_t *fn_step) {
    std::lock_guard<std::mutex> lk(g_jit_mu);
    const std::string key = std::to_string(device) + "\n" + src;
    auto it = g_jit_cache.find(key);
    if (it != g_jit_cache.end()) { *fn_step = it->second.fn_step; return it->second.fn; }
    hiprtcProgram prog = nullptr;
    const char *hdr_src[] = {k_src_rovmpc_h, k_src_device_math_h, k_src_rollout_kernels_h};
    const char *hdr_name[] = {"rovmpc.h", "device_math.h", "rollout_kernels.h"};
    hiprtcResult r = hiprtcCreateProgram(&prog, src.c_str(), "rovmpc_jit.hip", 3, hdr_src, hdr_name);
    if (r != HIPRTC_SUCCESS) { why = std::string("hiprtcCreateProgram: ") + hiprtcGetErrorString(r); return nullptr; }
#ifdef ROVMPC_STAMPS
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-DROVMPC_JIT_BUILD=1", "-DROVMPC_STAMPS=1"};   // diagnostic library
#else
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-DROVMPC_JIT_BUILD=1"};
#endif
    r = hiprtcCompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        why = std::string("hiprtcCompileProgram: ") + hiprtcGetErrorString(r) + ": " + log.substr(0, 300);
        hiprtcDestroyProgram(&prog);
        return nullptr;
    }
    size_t sz = 0;
    hiprtcGetCodeSize(prog, &sz);
    std::vector<char> code(sz);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    JitModule m;
    hipError_t e = hipModuleLoadData(&m.mod, code.data());
    if (e != hipSuccess) { why = std::string("hipModuleLoadData: ") + hipGetErrorString(e); return nullptr; }
    e = hipModuleGetFunction(&m.fn, m.mod, "rovmpc_rollout_jit");
    if (e != hipSuccess) { why = std::string("hipModuleGetFunction: ") + hipGetErrorString(e); (void)hipModuleUnload(m.mod); return nullptr; }
    if (hipModuleGetFunction(&m.fn_step, m.mod, "rovmpc_closed_loop_step_jit") != hipSuccess) m.fn_step = nullptr;
    g_jit_cache[key] = m;
    *fn_step = m.fn_step;
    return m.fn;
}

// What the rows' slot-dependency sets allow (generation-1 map; ROVMPC_JIT_NO_STRUCT=1 switches it off): see rollout_kernels.h.
static void jit_structure(const rovmpc_handle *h, const int32_t *code_th, int n_th, const int32_t *code_ga, int n_ga, int *gi, int *ts) {
    *gi = *ts = 0;
    if (h->cfg.feature_map != ROVMPC_FEATURES_GEN1 || getenv("ROVMPC_JIT_NO_STRUCT")) return;
    const unsigned dep_th = program_slots(code_th, n_th), dep_ga = program_slots(code_ga, n_ga);
    if ((dep_ga & ~((1u << 15) | (1u << 17))) == 0) *gi = 1;        // dgamma/dt on (gamma, gamma_prev) alone
    if ((dep_th & ((1u << 14) | (1u << 15))) == 0) *ts = 1;         // dtheta/dt blind to the stage state
    if (*ts && !*gi) *ts = 0;       // (measured: with gamma's stages still on the chain the split evaluations cost rows 5 / 9 0.4 us)
}

static std::string jit_source(const rovmpc_handle *h, const int32_t *code_th, int n_th, const int32_t *code_ga, int n_ga,
                              const double *consts, int gi, int ts, int ckc) {
    const char *real = h->cfg.dtype == ROVMPC_F64 ? "double" : "float";
    // the slots a stage sets itself (everything else is a row of a node, or the midpoint of two)
    const unsigned state_mask = h->cfg.feature_map == ROVMPC_FEATURES_GEN2 ? 0xf000u        // theta, gamma, cos theta, sin gamma
                              : h->cfg.feature_map == ROVMPC_FEATURES_GEN3 ? 0x3c00fu       // theta, gamma, their rates (+ the unused tail)
                                                                           : 0x3c000u;      // x14..x17: state and delay slots
    std::vector<std::string> subs, gsubs;
    const bool hoist = !getenv("ROVMPC_JIT_NO_HOIST");
    const std::string f_th = bytecode_to_cxx(code_th, n_th, consts, state_mask, hoist ? &subs : nullptr, (gi && hoist) ? &gsubs : nullptr, 1u << 17);
    const std::string f_ga = bytecode_to_cxx(code_ga, n_ga, consts, state_mask, hoist ? &subs : nullptr);
    std::string s;
    s += "#define ROVMPC_JIT_FMAP " + std::to_string(h->cfg.feature_map) + "\n";
    s += "#define ROVMPC_JIT_NSUB " + std::to_string(subs.size()) + "\n";
    s += "#define ROVMPC_JIT_CKC " + std::to_string(ckc) + "\n#define ROVMPC_JIT_N " + std::to_string((ckc && !getenv("ROVMPC_JIT_NO_NC")) ? h->cfg.N : 0) + "\n";      // candidates per workgroup as a literal (rollout_body, CKC)
    s += "#define ROVMPC_JIT_GI " + std::to_string(gi) + "\n#define ROVMPC_JIT_TS " + std::to_string(ts) + "\n";
    s += "#define ROVMPC_JIT_NGSUB " + std::to_string(gsubs.size()) + "\n";
    {
        bool has_sin = false;
        for (int pc = 0; pc < n_th; ++pc) has_sin = has_sin || (code_th[pc] & 0xff) == ROVMPC_OP_SIN;
        for (int pc = 0; pc < n_ga; ++pc) has_sin = has_sin || (code_ga[pc] & 0xff) == ROVMPC_OP_SIN;
        s += std::string("#define ROVMPC_JIT_PIN_TRIG ") + (has_sin ? "1" : "0") + "\n";
    }
    s += "#define ROVMPC_JIT_USED " + std::to_string(h->used_planes) + "u\n#include \"rollout_kernels.h\"\nnamespace rovmpc {\n";
    s += "template <typename T> RV_DEV T rv_sq(T a) { return a * a; }\n";
    s += "template <typename T> RV_DEV T rv_powi(T b, int e) { int ae = e < 0 ? -e : e; T r = T(1); "
         "while (ae) { if (ae & 1) r *= b; b *= b; ae >>= 1; } return e < 0 ? T(1) / r : r; }\n";
    s += std::string("template <> __device__ void jit_exo<") + real + ">(const " + real + " *x, " + real + " *e, const Trig<" + real + "> &tg) { typedef " + real + " T; (void)x; (void)e; (void)tg;";
    for (size_t k = 0; k < subs.size(); ++k) s += " e[" + std::to_string(k) + "] = " + subs[k] + ";";
    s += " }\n";
    s += std::string("template <> __device__ void jit_gsub<") + real + ">(const " + real + " *x, " + real + " *g, const Trig<" + real + "> &tg) { typedef " + real + " T; (void)x; (void)g; (void)tg;";
    for (size_t k = 0; k < gsubs.size(); ++k) s += " g[" + std::to_string(k) + "] = " + gsubs[k] + ";";
    s += " }\n";
    s += std::string("template <> __device__ ") + real + " jit_f_theta<" + real + ">(const " + real + " *x, const " + real + " *e, const " + real +
         " *g, const Trig<" + real + "> &tg) { typedef " + real + " T; (void)e; (void)g; (void)tg; return " + f_th + "; }\n";
    s += std::string("template <> __device__ ") + real + " jit_f_gamma<" + real + ">(const " + real + " *x, const " + real + " *e, const Trig<" + real + "> &tg) { typedef " + real +
         " T; (void)e; (void)tg; return " + f_ga + "; }\n";
    s += "}\nextern \"C\" __global__ void __launch_bounds__(512) rovmpc_rollout_jit(const rovmpc::RolloutArgs<" + std::string(real) +
         "> a) {\n    rovmpc::rollout_body<" + real + ", rovmpc::MODEL_JIT, " + std::to_string(h->cfg.vt_mode) + ", false, false, false, false, ROVMPC_JIT_CKC, ROVMPC_JIT_N>(a);\n}\n";
    s += "extern \"C\" __global__ void __launch_bounds__(512) rovmpc_closed_loop_step_jit(const rovmpc::RolloutArgs<" + std::string(real) +
         "> a, const rovmpc::HandoffArgs p) {\n    rovmpc::closed_loop_step_body<" + real + ", rovmpc::MODEL_JIT, " + std::to_string(h->cfg.vt_mode) + ", ROVMPC_JIT_CKC, ROVMPC_JIT_N>(a, p);\n}\n";
    if (getenv("ROVMPC_JIT_DUMP")) fprintf(stderr, "[rovmpc] hiprtc translation unit:\n%s\n", s.c_str());
    return s;
}

// ---- model ---------------------------------------------------------------------------------

// Static validation: opcodes known, indices in range, stack discipline, final depth 1.
const char *validate_code(const int32_t *code, int n, int n_feat, int n_consts) {
    if (n < 1 || n > ROVMPC_MAX_CODE) return "program length out of range";
    int sp = 0;
    for (int pc = 0; pc < n; ++pc) {
        int op = code[pc] & 0xff, arg = code[pc] >> 8;
        switch (op) {
        case ROVMPC_OP_PUSH_C: if (arg < 0 || arg >= n_consts) return "constant index out of range"; ++sp; break;
        case ROVMPC_OP_PUSH_F: if (arg < 0 || arg >= n_feat) return "feature index out of range"; ++sp; break;
        case ROVMPC_OP_ADD: case ROVMPC_OP_SUB: case ROVMPC_OP_MUL: case ROVMPC_OP_DIV: case ROVMPC_OP_POW:
            if (sp < 2) return "stack underflow"; --sp; break;
        case ROVMPC_OP_NEG: case ROVMPC_OP_SIN: case ROVMPC_OP_COS: case ROVMPC_OP_TANH: case ROVMPC_OP_ABS:
        case ROVMPC_OP_SQUARE: case ROVMPC_OP_EXP: case ROVMPC_OP_LOG: case ROVMPC_OP_SQRT: case ROVMPC_OP_POWI:
        case ROVMPC_OP_SAFE_LOG: case ROVMPC_OP_SAFE_SQRT:
            if (sp < 1) return "stack underflow"; break;
        default: return "unknown opcode";
        }
        if (sp > ROVMPC_MAX_STACK) return "expression needs more than ROVMPC_MAX_STACK operands";
    }
    return sp == 1 ? nullptr : "program does not leave exactly one value";
}

// Structural recognition of the reference's chosen rows.  The bytecode is evaluated over the algebra of affine forms
// sum_i c_i * atom_i with atoms {1, x_j, sin(x_j)}: constants and features push one-term forms, + - combine terms, * and /
// need a pure constant on one side (the right side for /), sin needs its argument to be exactly one feature.  Any other
// operator, or a product of two non-constant forms, ends the recognition (the model is then NOT the compiled-in one, whatever
// it evaluates to).  Two programs with the same term list are the same function on all of R^18, so this decides identity
// exactly -- no sample points, no tolerance on values; the coefficients must be the published 0.048152514 to the last bit
// (the CSV's `equation` form and its expanded `sympy_format` form both give exactly that).
typedef std::map<int, double> AffineForm;            // atom id -> coefficient; id 0 = 1, 1 + j = x_j, 100 + j = sin(x_j)
static bool affine_of(const int32_t *code, int n, const double *consts, AffineForm &out) {
    std::vector<AffineForm> st;
    auto is_const = [](const AffineForm &f) { for (auto &t : f) if (t.first != 0 && t.second != 0.0) return false; return true; };
    auto const_of = [](const AffineForm &f) { auto it = f.find(0); return it == f.end() ? 0.0 : it->second; };
    for (int pc = 0; pc < n; ++pc) {
        const int op = code[pc] & 0xff, arg = code[pc] >> 8;
        if (op == ROVMPC_OP_PUSH_C) { st.push_back({{0, consts[arg]}}); continue; }
        if (op == ROVMPC_OP_PUSH_F) { st.push_back({{1 + arg, 1.0}}); continue; }
        if (op == ROVMPC_OP_NEG) { for (auto &t : st.back()) t.second = -t.second; continue; }
        if (op == ROVMPC_OP_SIN) {
            AffineForm &f = st.back();
            int feat = -1; bool ok = true;
            for (auto &t : f) { if (t.second == 0.0) continue; if (t.first >= 1 && t.first < 100 && t.second == 1.0 && feat < 0) feat = t.first - 1; else ok = false; }
            if (!ok || feat < 0) return false;
            f = {{100 + feat, 1.0}};
            continue;
        }
        if (op == ROVMPC_OP_ADD || op == ROVMPC_OP_SUB || op == ROVMPC_OP_MUL || op == ROVMPC_OP_DIV) {
            AffineForm b = st.back(); st.pop_back();
            AffineForm &a = st.back();
            if (op == ROVMPC_OP_ADD || op == ROVMPC_OP_SUB) {
                for (auto &t : b) a[t.first] += op == ROVMPC_OP_ADD ? t.second : -t.second;
            } else if (op == ROVMPC_OP_MUL) {
                if (is_const(b)) { const double c = const_of(b); for (auto &t : a) t.second *= c; }
                else if (is_const(a)) { const double c = const_of(a); a = b; for (auto &t : a) t.second *= c; }
                else return false;
            } else {
                if (!is_const(b)) return false;
                const double c = const_of(b); for (auto &t : a) t.second /= c;
            }
            continue;
        }
        return false;
    }
    if (st.size() != 1) return false;
    out.clear();
    for (auto &t : st[0]) if (t.second != 0.0) out[t.first] = t.second;
    return true;
}
static bool is_reference_rows(const int32_t *code_th, int n_th, const int32_t *code_ga, int n_ga, const double *consts) {
    AffineForm th, ga;
    if (!affine_of(code_th, n_th, consts, th) || !affine_of(code_ga, n_ga, consts, ga)) return false;
    const double KT = 0.048152514;
    const AffineForm want_th = {{1 + 16, -KT}, {1 + 3, -KT}, {100 + 17, KT}, {100 + 3, -KT}};
    const AffineForm want_ga = {{1 + 15, 1.0}, {1 + 17, -1.0}};
    return th == want_th && ga == want_ga;
}

extern "C" int rovmpc_set_model(rovmpc_handle *h, int32_t n_features, const double *mean, const double *scale,
                                const int32_t *code_theta, int32_t n_code_theta, const int32_t *code_gamma,
                                int32_t n_code_gamma, const double *consts, int32_t n_consts) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!mean || !scale || !code_theta || !code_gamma || (n_consts > 0 && !consts))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_model: null argument");
    if (n_features < 1 || n_features > ROVMPC_MAX_FEATURES) FAIL(h, ROVMPC_ERR_INVALID, "n_features out of range");
    if (n_consts < 0 || n_consts > ROVMPC_MAX_CODE) FAIL(h, ROVMPC_ERR_INVALID, "n_consts out of range");
    const char *why;
    if ((why = validate_code(code_theta, n_code_theta, n_features, n_consts))) FAIL(h, ROVMPC_ERR_INVALID, "theta program: %s", why);
    if ((why = validate_code(code_gamma, n_code_gamma, n_features, n_consts))) FAIL(h, ROVMPC_ERR_INVALID, "gamma program: %s", why);
    for (int i = 0; i < n_features; ++i)
        if (!(scale[i] != 0.0) || !isfinite(scale[i]) || !isfinite(mean[i])) FAIL(h, ROVMPC_ERR_INVALID, "scaler entry %d is not finite / zero scale", i);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->n_feat = n_features;
    memcpy(h->mean, mean, n_features * sizeof(double));
    memcpy(h->scale, scale, n_features * sizeof(double));
    h->n_th = n_code_theta; h->n_ga = n_code_gamma; h->n_consts = n_consts;
    HIPCHK(h, hipMemcpy(h->d_code_th, code_theta, n_code_theta * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_code_ga, code_gamma, n_code_gamma * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_consts > 0) {
        HIPCHK(h, hipMemcpy(h->d_consts64, consts, n_consts * sizeof(double), hipMemcpyHostToDevice));
        if (h->cfg.dtype == ROVMPC_F64) {
            HIPCHK(h, hipMemcpy(h->d_consts, consts, n_consts * sizeof(double), hipMemcpyHostToDevice));
        } else {
            std::vector<float> cf(consts, consts + n_consts);
            HIPCHK(h, hipMemcpy(h->d_consts, cf.data(), n_consts * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (h->cfg.dtype == ROVMPC_F64) {
        RolloutConsts<double> k;
        fill_consts<double>(h, k);
        HIPCHK(h, hipMemcpy(h->d_k, &k, sizeof(k), hipMemcpyHostToDevice));
    } else {
        RolloutConsts<float> k;
        fill_consts<float>(h, k);
        HIPCHK(h, hipMemcpy(h->d_k, &k, sizeof(k), hipMemcpyHostToDevice));
    }
    // The compiled-in kernel is substituted only for a model that IS the reference's chosen rows
    // (saved_models/equations_*.csv complexity 13: ((((sin(x17) - sin(x3)) - x16) - x3) * 0.048152514); complexity 3:
    // x15 - x17), decided structurally -- see is_reference_rows -- never by sampling the functions.
    const bool same = n_features == 18 && !h->cfg.force_interpreter && !h->cfg.no_builtin &&
                      h->cfg.feature_map == ROVMPC_FEATURES_GEN1 &&
                      is_reference_rows(code_theta, n_code_theta, code_gamma, n_code_gamma, consts);
    {
        // exogenous planes the expressions read (plane 13 = angle_proj: feature 13, or 16 in generation 2)
        unsigned m = 0;
        auto scan = [&](const int32_t *code, int n) {
            for (int pc = 0; pc < n; ++pc)
                if ((code[pc] & 0xff) == ROVMPC_OP_PUSH_F) {
                    const int f = code[pc] >> 8;
                    if (h->cfg.feature_map == ROVMPC_FEATURES_GEN2) { if (f < 12) m |= 1u << f; else if (f == 16) m |= 1u << 13; }
                    else if (h->cfg.feature_map == ROVMPC_FEATURES_GEN3) { if (f >= 4 && f < 14) m |= 1u << (f - 4); }   // plane p = slot 4 + p
                    else if (f < 14) m |= 1u << f;
                }
        };
        scan(code_theta, n_code_theta); scan(code_gamma, n_code_gamma);
        h->used_planes = m;
    }
    h->builtin = same;
    h->model_kind = same ? MODEL_BUILTIN : MODEL_INTERP;
    h->jit_fn = nullptr; h->jit_fn_step = nullptr; h->jit_gi = 0; h->jit_ts = 0; h->jit_ckc = 0;
    h->err.clear();
    if (!same && !h->cfg.force_interpreter && !h->cfg.jit_off && n_features <= 18) {
        std::string why;
        int gi = 0, ts = 0;
        jit_structure(h, code_theta, n_code_theta, code_gamma, n_code_gamma, &gi, &ts);
        // the geometry this model will run with (configure_geometry below decides the same): 16 candidates per workgroup
        // become a literal of the module
        hipDeviceProp_t prop{};
        if (hipGetDeviceProperties(&prop, h->cfg.device) == hipSuccess && prop.multiProcessorCount > 0) h->n_cu = prop.multiProcessorCount;
        const int ck_jit = pick_ck(&h->cfg, MODEL_JIT, jit_lds_planes(h->used_planes, h->cfg.vt_mode, h->cfg.feature_map), h->n_cu, gi);
        const int ckc = (ck_jit == 16 && !getenv("ROVMPC_JIT_NO_CKC")) ? 16 : 0;
        const std::string src = jit_source(h, code_theta, n_code_theta, code_gamma, n_code_gamma, consts, gi, ts, ckc);
        hipFunction_t fn = jit_build(h->cfg.device, src, why, &h->jit_fn_step);
        if (fn) { h->jit_fn = fn; h->model_kind = MODEL_JIT; h->jit_gi = gi; h->jit_ts = ts; h->jit_ckc = ckc; }
        else h->err = "hiprtc specialisation unavailable, using the bytecode interpreter: " + why;
    }
    if (const char *why = configure_geometry(h, h->model_kind)) FAIL(h, ROVMPC_ERR_INVALID, "%s", why);
    if (h->model_kind == MODEL_JIT && h->jit_ckc && h->CK != h->jit_ckc) FAIL(h, ROVMPC_ERR_INVALID, "internal: the specialised module was built for %d candidates per workgroup, the geometry has %d", h->jit_ckc, h->CK);
    h->has_model = true;
    return ROVMPC_OK;
}

extern "C" int32_t rovmpc_model_path(const rovmpc_handle *h) { return h ? h->model_kind : -1; }
extern "C" int32_t rovmpc_model_structure(const rovmpc_handle *h) { return (h && h->model_kind == MODEL_JIT) ? (h->jit_gi | (h->jit_ts << 1)) : 0; }
extern "C" int32_t rovmpc_closed_loop_form(const rovmpc_handle *h) { return h ? h->cl_form : -1; }

extern "C" int rovmpc_set_rotation_table(rovmpc_handle *h, const double *R) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!R) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_rotation_table: null R");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)h->cfg.N * 9;
    if (h->cfg.dtype == ROVMPC_F64) {
        HIPCHK(h, hipMemcpy(h->d_Rtab, R, n * sizeof(double), hipMemcpyHostToDevice));
    } else {
        std::vector<float> rf(R, R + n);
        HIPCHK(h, hipMemcpy(h->d_Rtab, rf.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
    h->has_rtab = true;
    return ROVMPC_OK;
}

// ---- launches -------------------------------------------------------------------------------

// The argument block of one launch from the handle's model, workspace and geometry and from the launch's own options.  The
// epoch is left to launch_rollout: an argument block that is never launched (a probe) takes none.
template <typename T> void fill_args(const rovmpc_handle *h, RolloutArgs<T> &a, const double *d_state, const void *d_U,
                                     double *d_result, const Geo &g, const StepOpts &o) {
    const rovmpc_config &c = h->cfg;
    const int B = o.B;
    a.U = (const T *)d_U; a.state = d_state; a.k = (const RolloutConsts<T> *)h->d_k;
    a.code_th = h->d_code_th; a.code_ga = h->d_code_ga;
    a.consts = (const T *)h->d_consts; a.Rtab = (const T *)h->d_Rtab;
    a.J = (T *)(o.J ? o.J : B > 1 ? h->d_Jb : h->d_J); a.traj_all = (T *)o.traj_all;
    a.blk_traj = B > 1 ? h->d_blk_trajb : h->d_blk_traj;
    a.result = d_result; a.k_offset = o.k_offset; a.slots = o.slots; a.rank = o.rank; a.world = o.world;
    a.N = c.N; a.K = c.K; a.CK = g.CK; a.M = c.n_shape_pts; a.n_th = h->n_th; a.n_ga = h->n_ga;
    a.prev_mode = c.prev_mode; a.integrator = c.integrator; a.debug = c.debug_flags; a.fmap = c.feature_map;
    a.used_planes = h->used_planes;
    a.ck_shift = 0;
    while ((1 << a.ck_shift) < g.CK) ++a.ck_shift;
    a.magic_3n = (unsigned)(4294967296ULL / (unsigned long long)(3 * c.N)) + 1u;
    a.granules = B > 1 ? h->d_granulesb : h->d_granules;
    a.sweeper = (long long)B * g.nblocks <= h->n_cu ? 0 : g.nblocks - 1;
    a.epoch = 0;
    a.NT = g.NT; a.nblocks = g.nblocks;
    a.plant_next = o.plant_next; a.plant_state = o.plant_state; a.plant_feedback = o.plant_feedback;
    a.ring = nullptr; a.exo_cur = nullptr; a.seq_theta = nullptr; a.seq_gamma = nullptr;
    a.samp_seed = 0; a.samp_step = 0; a.samp_warm = nullptr; a.samp_best = nullptr; a.samp_blk_u = nullptr;
    a.step = 0; a.from_ring = 0; a.wait_theta = 0; a.publish = 0;
    a.result_host = o.result_host; a.done_flag = o.done_flag; a.done_seq = o.done_seq;
    a.flag_consumed = o.flag_consumed; a.flag_rolled = o.flag_rolled;
    a.consumed_need = o.consumed_need; a.rolled_seq = o.rolled_seq;
    a.slot_bad = o.slot_bad; a.err = h->d_err; a.inject = o.inject;
    a.handoff_ticks = (unsigned long long)(h->handoff_timeout_ms * 1e5);      // 100 MHz clock
    a.stamps = h->d_stamps;
    // (single-problem launches only: a batch has a gamma path per problem)
    static const bool no_gtab = getenv("ROVMPC_NO_GTAB") != nullptr;          // (diagnosis: every workgroup integrates gamma itself)
    a.gtab = (B == 1 && !no_gtab) ? (T *)h->d_gtab : nullptr;
    a.gtab_tag = B == 1 ? (unsigned long long *)((char *)h->d_gtab + (size_t)8 * (c.N + 1) * 8) : nullptr;
}
template void fill_args<double>(const rovmpc_handle *, RolloutArgs<double> &, const double *, const void *, double *, const Geo &, const StepOpts &);
template void fill_args<float>(const rovmpc_handle *, RolloutArgs<float> &, const double *, const void *, double *, const Geo &, const StepOpts &);

// What a launch of `kind` with geometry g and options o runs on this handle: the instance or the hiprtc function, with its
// dynamic LDS; a kernel that needs more than 64 KiB of it is told so here.  ROVMPC_NO_LITERAL_N=1 keeps the horizon a run-time
// value (read per call: the parity tests switch it inside one process).
hipError_t rollout_launchable(const rovmpc_handle *h, LaunchKind kind, const Geo &g, const StepOpts &o, Launchable &k) {
    const rovmpc_config &c = h->cfg;
    k = Launchable();
    if (h->model_kind == MODEL_JIT) {
        k.mod = kind == LAUNCH_PLAIN ? h->jit_fn : kind == LAUNCH_STEP ? h->jit_fn_step : nullptr;
        k.lds = lds_need(&c, g.CK, MODEL_JIT, jit_lds_planes(h->used_planes, c.vt_mode, c.feature_map), h->jit_gi);
        if (!k.mod) return hipErrorInvalidDeviceFunction;
        if (k.lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)k.mod, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
        return hipSuccess;
    }
    const bool builtin = h->model_kind == MODEL_BUILTIN;
    k.fn = compiled_instance(c, h->model_kind, {kind, c.N, g.CK, o.lean(), builtin && !getenv("ROVMPC_NO_LITERAL_N")});
    k.lds = lds_need(&c, g.CK, h->model_kind);
    if (!k.fn) return hipErrorInvalidDeviceFunction;
    if (k.lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
        if (e != hipSuccess) return e;
    }
#ifdef ROVMPC_STAMPS
    static bool told = false;
    if (!told && kind == LAUNCH_PLAIN && getenv("ROVMPC_DIAG_OCCUPANCY")) {
        told = true;
        int nb = -1; hipFuncAttributes fa{};
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, g.NT, k.lds);
        hipFuncGetAttributes(&fa, k.fn);
        fprintf(stderr, "[rovmpc diag] NT %d lds %zu: resident workgroups/CU %d; regs %d static lds %zu scratch %zu maxThreads %d\n",
                g.NT, k.lds, nb, fa.numRegs, fa.sharedSizeBytes, fa.localSizeBytes, fa.maxThreadsPerBlock);
    }
#endif
    return hipSuccess;
}

// Workgroups of k the device holds at once with NT threads each: resident workgroups per CU x CUs.
hipError_t launchable_capacity(const rovmpc_handle *h, const Launchable &k, int NT, int *capacity) {
    int per_cu = 0;
    const hipError_t e = k.mod ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.mod, NT, k.lds)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, NT, k.lds);
    *capacity = e == hipSuccess ? per_cu * h->n_cu : 0;
    return e;
}

// The launch itself; it takes the launch epoch (the tag of the granules this launch writes).  p: the second argument of the
// closed-loop step kernels.
template <typename T> hipError_t launch_rollout(const rovmpc_handle *h, const Launchable &k, RolloutArgs<T> &a, int B, hipStream_t s,
                                                const HandoffArgs *p) {
    if (++*h->epoch_ctr == 0) ++*h->epoch_ctr;      // never 0 (the granules start zeroed)
    a.epoch = *h->epoch_ctr;
    if (k.mod) {
        struct { RolloutArgs<T> a; HandoffArgs p; } both;
        void *buf = &a;
        size_t asz = sizeof(a);
        if (p) { both.a = a; both.p = *p; buf = &both; asz = sizeof(both); }
        void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, buf, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
        return hipModuleLaunchKernel(k.mod, a.nblocks, B, 1, a.NT, 1, 1, (unsigned)k.lds, s, nullptr, extra);
    }
    void *args[] = {&a, const_cast<HandoffArgs *>(p)};
    (void)hipLaunchKernel(k.fn, dim3(a.nblocks, B), dim3(a.NT), args, k.lds, s);
    return hipGetLastError();
}
template hipError_t launch_rollout<double>(const rovmpc_handle *, const Launchable &, RolloutArgs<double> &, int, hipStream_t, const HandoffArgs *);
template hipError_t launch_rollout<float>(const rovmpc_handle *, const Launchable &, RolloutArgs<float> &, int, hipStream_t, const HandoffArgs *);

int check_ready(rovmpc_handle *h) {
    if (!h->has_model) FAIL(h, ROVMPC_ERR_NO_MODEL, "rovmpc_set_model has not been called");
    const int want = h->cfg.feature_map == ROVMPC_FEATURES_GEN2 ? 17 : h->cfg.feature_map == ROVMPC_FEATURES_GEN3 ? 14 : 18;
    if (h->n_feat != want)
        FAIL(h, ROVMPC_ERR_UNSUPPORTED, "feature_map %d has %d slots (simply.py:15-41 / simulate_rk4_theta_gamma.py:12-42 / main_fun.py:849-864) but the model has %d",
             h->cfg.feature_map, want, h->n_feat);
    if (h->cfg.vt_mode == ROVMPC_VT_TABLE && !h->has_rtab) FAIL(h, ROVMPC_ERR_INVALID, "vt_mode TABLE needs rovmpc_set_rotation_table");
    return ROVMPC_OK;
}

template <typename T> static hipError_t launch_plain_t(const rovmpc_handle *h, const double *d_state, const void *d_U, double *d_result,
                                                       hipStream_t s, const StepOpts &o) {
    RolloutArgs<T> a;
    Launchable k;
    const Geo g = launch_geometry(h, o.B);
    fill_args<T>(h, a, d_state, d_U, d_result, g, o);
    const hipError_t e = rollout_launchable(h, LAUNCH_PLAIN, g, o, k);
    return e != hipSuccess ? e : launch_rollout<T>(h, k, a, o.B, s);
}

int enqueue_step(rovmpc_handle *h, const double *d_state, const void *d_U, double *d_result, hipStream_t s, const StepOpts &o) {
    int rc = check_ready(h);
    if (rc) return rc;
    const bool time_it = h->timing && h->ev_used + 2 <= (int)h->ev.size();
    if (time_it) HIPCHK(h, hipEventRecord(h->ev[h->ev_used], s));
    hipError_t e = h->cfg.dtype == ROVMPC_F64 ? launch_plain_t<double>(h, d_state, d_U, d_result, s, o)
                                              : launch_plain_t<float>(h, d_state, d_U, d_result, s, o);
    if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "rollout kernel launch failed: %s", hipGetErrorString(e));
    if (!o.J) h->last_batch = o.B;                  // (rovmpc_batch_costs_device: the last launch that wrote the handle's own costs)
    if (time_it) { HIPCHK(h, hipEventRecord(h->ev[h->ev_used + 1], s)); h->ev_used += 2; }
    return ROVMPC_OK;
}

extern "C" int rovmpc_step_device(rovmpc_handle *h, const double *d_state, const void *d_U, double *d_result, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!d_state || !d_U || !d_result) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_step_device: null pointer");
    return enqueue_step(h, d_state, d_U, d_result, (hipStream_t)stream);
}

// Workspace of a batched launch: costs, per-workgroup trajectories and hand-off granules for B problems.  The larger set is
// made before the old one is let go, so a failed allocation leaves the handle with the workspace and capacity it had.
static int ensure_batch(rovmpc_handle *h, int B) {
    if (B <= h->batch_cap) return ROVMPC_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const rovmpc_config &c = h->cfg;
    const size_t max_blocks = c.candidates_per_block > 0 ? (size_t)((c.K + c.candidates_per_block - 1) / c.candidates_per_block) : (size_t)c.K;
    const size_t gran_bytes = (size_t)B * gran_stride((int)max_blocks, c.N) * sizeof(unsigned long long);
    void *fresh[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipMalloc(&fresh[0], (size_t)B * c.K * h->esz);
    if (e == hipSuccess) e = hipMalloc(&fresh[1], (size_t)B * max_blocks * (c.N + 1) * 2 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&fresh[2], gran_bytes);
    if (e == hipSuccess) e = hipMemset(fresh[2], 0, gran_bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();  // nothing may still be using the old buffers
    if (e != hipSuccess) {
        for (void *p : fresh) if (p) (void)hipFree(p);
        (void)hipGetLastError();                     // an allocation failure is not sticky: the handle stays usable
        FAIL(h, ROVMPC_ERR_HIP, "batched workspace for %d problems: %s", B, hipGetErrorString(e));
    }
    void *old[] = {h->d_Jb, h->d_blk_trajb, h->d_granulesb};
    for (void *p : old) if (p) (void)hipFree(p);
    h->d_Jb = fresh[0]; h->d_blk_trajb = (double *)fresh[1]; h->d_granulesb = (unsigned long long *)fresh[2];
    h->batch_cap = B;
    return ROVMPC_OK;
}

extern "C" int rovmpc_step_batch_device(rovmpc_handle *h, int32_t B, const double *d_states, const void *d_U, double *d_results,
                                        void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (B < 1 || B > 65535) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_step_batch_device: B must be in 1..65535 (got %d)", B);
    if (!d_states || !d_U || !d_results) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_step_batch_device: null pointer");
    if (B == 1) return enqueue_step(h, d_states, d_U, d_results, (hipStream_t)stream);
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = ensure_batch(h, B))) return rc;
    StepOpts o;
    o.B = B;
    return enqueue_step(h, d_states, d_U, d_results, (hipStream_t)stream, o);
}

extern "C" int rovmpc_batch_costs_device(rovmpc_handle *h, const void **d_J) {
    if (!h || !d_J) return ROVMPC_ERR_INVALID;
    *d_J = h->last_batch > 1 ? h->d_Jb : h->d_J;        // where the last launch on this handle wrote its costs
    return ROVMPC_OK;
}

// Error word of the handle (non-blocking): 0 = nothing raised; otherwise ROVMPC_ERR_HIP with the reason, and the word is
// cleared.  Only meaningful for work the host has already synchronised with.
static int take_device_errors(rovmpc_handle *h) {
    if (!h->h_err) return ROVMPC_OK;
    const unsigned e = __atomic_exchange_n(h->h_err, 0u, __ATOMIC_ACQ_REL);
    if (!e) return ROVMPC_OK;
    FAIL(h, ROVMPC_ERR_HIP, "GPU-side hand-off gave up:%s%s%s -- the affected step's record carries a NaN cost",
         (e & ERR_WAIT_ROLLED) ? " [a collective never saw its rollout's row]" : "",
         (e & ERR_CONSUMED) ? " [a rollout never saw the select that frees its slot row]" : "",
         (e & ERR_SWEEP) ? " [the arg-min sweep never saw a workgroup's record]" : "");
}

// ---- MPC.step with the candidates drawn on the GPU: one call, no copies on the step path ---------------------------
static int ensure_sampler(rovmpc_handle *h) {
    const size_t ub = (size_t)h->cfg.K * h->cfg.N * 3 * h->esz;
    for (void *&d_U : h->d_Us)
        if (!d_U) HIPCHK(h, hipMalloc(&d_U, ub));
    return h->samp_box.d_done ? ROVMPC_OK : mailbox_alloc(h, h->samp_box, (size_t)rovmpc_result_len(h));
}

// The kernel that ends a step releases `seq` into the mailbox behind its results: spin on the word (a stream synchronise
// costs several microseconds of wake-up latency); after ~2 s fall back to the blocking call so a failed launch is reported.
static int mailbox_wait(rovmpc_handle *h, const Mailbox &m, unsigned long long seq, const char *what) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(m.h_done, __ATOMIC_ACQUIRE) == seq) return ROVMPC_OK;
        if ((spins & 0xffff) == 0xffff && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (__atomic_load_n(m.h_done, __ATOMIC_ACQUIRE) != seq) FAIL(h, ROVMPC_ERR_HIP, "the %s finished without publishing its record", what);
            return ROVMPC_OK;
        }
    }
}

int launched(rovmpc_handle *h, const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return ROVMPC_OK;
}

// kern<T, QC> of an update: T by the handle's dtype, QC = 4 columns per thread where a row is wider than the workgroup
#define LAUNCH_T_QC(kern, h, wide, ...)                                                                                       \
    do {                                                                                                                      \
        if ((h)->cfg.dtype == ROVMPC_F64) { if (wide) hipLaunchKernelGGL((kern<double, 4>), __VA_ARGS__); else hipLaunchKernelGGL((kern<double, 1>), __VA_ARGS__); } \
        else { if (wide) hipLaunchKernelGGL((kern<float, 4>), __VA_ARGS__); else hipLaunchKernelGGL((kern<float, 1>), __VA_ARGS__); } \
    } while (0)

// grid of the samplers: 256 threads, four elements of the tensor each
static const int SAMPLER_NT = 256;
static int sampler_grid(long long total) { return (int)(((total + 3) / 4 + SAMPLER_NT - 1) / SAMPLER_NT); }

static int launch_sampler(rovmpc_handle *h, const rovmpc_state *state, uint64_t seed, uint64_t step, const double *mean3,
                          const double *std3, int warm, void *d_U, const void *d_Uprev, hipStream_t s, const double *warm_seq = nullptr) {
    SampleArgs sa;
    memset(&sa, 0, sizeof(sa));
    if (state) { sa.state = *state; sa.d_state = h->d_state; }
    sa.seed = seed; sa.step = step;
    for (int i = 0; i < 3; ++i) { sa.mean[i] = mean3[i]; sa.std[i] = std3[i]; }
    sa.total = (long long)h->cfg.K * h->cfg.N * 3; sa.N = h->cfg.N;
    sa.warm = warm; sa.Uprev = d_Uprev; sa.prev_record = h->d_result; sa.warm_seq = warm_seq;
    const dim3 grid(sampler_grid(sa.total)), bs(SAMPLER_NT);
    if (h->cfg.dtype == ROVMPC_F64) hipLaunchKernelGGL(sample_candidates_kernel<double>, grid, bs, 0, s, sa, (double *)d_U);
    else hipLaunchKernelGGL(sample_candidates_kernel<float>, grid, bs, 0, s, sa, (float *)d_U);
    return launched(h, "sampler");
}

extern "C" int rovmpc_sample_candidates_device(rovmpc_handle *h, uint64_t seed, uint64_t step, const double *mean3,
                                               const double *std3, void *d_U, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!mean3 || !std3 || !d_U) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_sample_candidates_device: null pointer");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return launch_sampler(h, nullptr, seed, step, mean3, std3, 0, d_U, nullptr, (hipStream_t)stream);
}

// Compiled-in model: the rollout kernel draws its candidates itself (rollout_kernel_sampled) -- no sampler launch, no
// candidate tensor, the state in the kernel arguments.
template <typename T>
static int fused_sampled_step_t(rovmpc_handle *h, const rovmpc_state *state, uint64_t seed, uint64_t step, const double *mean3,
                                const double *std3, int warm, const StepOpts &o) {
    const int cur = (int)(h->samp_steps & 1);
    const size_t row = (size_t)h->cfg.N * 3;
    RolloutArgs<T> a;
    Launchable k;
    const Geo g = launch_geometry(h, 1);
    fill_args<T>(h, a, h->d_state, nullptr, h->d_result, g, o);
    a.samp_seed = seed; a.samp_step = step;
    for (int i = 0; i < 3; ++i) { a.samp_mean[i] = mean3[i]; a.samp_std[i] = std3[i]; }
    a.samp_warm = warm ? h->d_best + (size_t)(cur ^ 1) * row : nullptr;
    a.samp_best = h->d_best + (size_t)cur * row;
    a.samp_blk_u = h->d_blk_u;
    memcpy(a.samp_state, state, sizeof(a.samp_state));
    hipError_t e = rollout_launchable(h, LAUNCH_SAMPLED, g, o, k);
    if (e == hipSuccess) e = launch_rollout<T>(h, k, a, 1, h->stream);
    if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "fused sampling launch failed: %s", hipGetErrorString(e));
    return ROVMPC_OK;
}

extern "C" int rovmpc_mpc_step_sampled(rovmpc_handle *h, const rovmpc_state *state, uint64_t seed, uint64_t step,
                                       const double *mean3, const double *std3, int32_t warm_start, double *record_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!state || !mean3 || !std3 || !record_out) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mpc_step_sampled: null pointer");
    int rc = check_ready(h);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = ensure_sampler(h))) return rc;
    const int cur = (int)(h->samp_steps & 1);
    const int warm = warm_start && h->samp_steps > 0;
    const bool fused = h->model_kind == MODEL_BUILTIN && (h->samp_steps == 0 || h->last_fused) && !h->timing;
    // a fused step keeps its winner's sequence in d_best only (the candidate tensor never exists): when the handle leaves the
    // fused path -- rovmpc_timing_enable, or rovmpc_set_model with another model -- the next step's warm start reads it there
    const bool prev_fused = h->samp_steps > 0 && h->last_fused;
    h->last_seed = seed; h->last_step = step; h->last_warm = warm; h->last_fused = fused;
    for (int i = 0; i < 3; ++i) { h->last_mean[i] = mean3[i]; h->last_std[i] = std3[i]; }
    const unsigned long long seq = h->samp_steps + 1;
    StepOpts o;                                  // either way the step publishes its record into the sampled step's mailbox
    o.result_host = h->samp_box.d_out; o.done_flag = h->samp_box.d_done; o.done_seq = seq;
    if (fused) {
        if (!h->d_best) {
            const size_t max_blocks = h->cfg.candidates_per_block > 0 ? (size_t)((h->cfg.K + h->cfg.candidates_per_block - 1) / h->cfg.candidates_per_block) : (size_t)h->cfg.K;
            HIPCHK(h, hipMalloc((void **)&h->d_best, (size_t)2 * h->cfg.N * 3 * sizeof(double)));
            // (tagged granules, two per double: zeroed once, epoch 0 is never a valid tag)
            // (then the slow tail's plane of plain doubles, 3 N per workgroup)
            HIPCHK(h, hipMalloc((void **)&h->d_blk_u, max_blocks * (size_t)h->cfg.N * 9 * sizeof(unsigned long long)));
            HIPCHK(h, hipMemset(h->d_blk_u, 0, max_blocks * (size_t)h->cfg.N * 9 * sizeof(unsigned long long)));
        }
        rc = h->cfg.dtype == ROVMPC_F64 ? fused_sampled_step_t<double>(h, state, seed, step, mean3, std3, warm, o)
                                        : fused_sampled_step_t<float>(h, state, seed, step, mean3, std3, warm, o);
        ++h->samp_steps;
        if (rc) return rc;
    } else {
        const double *warm_seq = (warm && prev_fused) ? h->d_best + (size_t)(cur ^ 1) * h->cfg.N * 3 : nullptr;
        if ((rc = launch_sampler(h, state, seed, step, mean3, std3, warm, h->d_Us[cur], h->d_Us[cur ^ 1], h->stream, warm_seq))) return rc;
        ++h->samp_steps;
        if ((rc = enqueue_step(h, h->d_state, h->d_Us[cur], h->d_result, h->stream, o))) return rc;
    }
    if ((rc = mailbox_wait(h, h->samp_box, seq, "step"))) return rc;
    memcpy(record_out, h->samp_box.h_out, (size_t)rovmpc_result_len(h) * sizeof(double));
    return take_device_errors(h);
}

extern "C" int rovmpc_sampled_candidates(rovmpc_handle *h, void *U_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!U_out || h->samp_steps == 0) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_sampled_candidates: no sampled step yet");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int cur = (int)((h->samp_steps - 1) & 1);
    if (h->last_fused) {
        // the fused step never stored its tensor: draw it again with the stand-alone sampler (same routine, same bits),
        // warm start from the previous winner's sequence, which the step left untouched
        const double *warm_seq = h->last_warm ? h->d_best + (size_t)(cur ^ 1) * h->cfg.N * 3 : nullptr;
        int rc = launch_sampler(h, nullptr, h->last_seed, h->last_step, h->last_mean, h->last_std, h->last_warm, h->d_Us[cur], nullptr, h->stream, warm_seq);
        if (rc) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    HIPCHK(h, hipMemcpy(U_out, h->d_Us[cur], (size_t)h->cfg.K * h->cfg.N * 3 * h->esz, hipMemcpyDeviceToHost));
    return ROVMPC_OK;
}

extern "C" int rovmpc_device_status(rovmpc_handle *h) {
    if (!h) return ROVMPC_ERR_INVALID;
    return take_device_errors(h);
}

extern "C" int rovmpc_set_option(rovmpc_handle *h, const char *name, double value) {
    if (!h || !name) return ROVMPC_ERR_INVALID;
    if (!strcmp(name, "handoff_timeout_ms")) {
        if (!(value > 0) || value > 600000.0) FAIL(h, ROVMPC_ERR_INVALID, "handoff_timeout_ms must be in (0, 600000]");
        h->handoff_timeout_ms = value;
    } else if (!strcmp(name, "track_chunk")) {
        if (!(value >= 1) || value > 65536.0 || value != (double)(int)value) FAIL(h, ROVMPC_ERR_INVALID, "track_chunk must be an integer in 1..65536");
        h->track_chunk = (int)value;
    } else if (!strcmp(name, "inject_skip_rolled")) {
        h->inject_skip_rolled = (int)value;
    } else if (!strcmp(name, "inject_skip_consumed")) {
        h->inject_skip_consumed = (int)value;
    } else {
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_option: unknown option '%s'", name);
    }
    return ROVMPC_OK;
}

extern "C" int rovmpc_step_device_sharded(rovmpc_handle *h, const double *d_state, const void *d_U, int64_t k_offset,
                                          int32_t rank, int32_t world, int64_t *d_slots, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!d_state || !d_U || !d_slots) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_step_device_sharded: null pointer");
    if (world < 1 || rank < 0 || rank >= world) FAIL(h, ROVMPC_ERR_INVALID, "bad rank/world %d/%d", rank, world);
    StepOpts o;
    o.k_offset = k_offset; o.slots = (long long *)d_slots; o.rank = rank; o.world = world;
    return enqueue_step(h, d_state, d_U, h->d_result, (hipStream_t)stream, o);
}

extern "C" int rovmpc_select_device(rovmpc_handle *h, const int64_t *d_slots, int32_t world, double *d_result, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!d_slots || !d_result || world < 1) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_select_device: bad argument");
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const long long *)d_slots, world,
                       rovmpc_result_len(h), d_result);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) FAIL(h, ROVMPC_ERR_HIP, "select kernel launch failed: %s", hipGetErrorString(e));
    return ROVMPC_OK;
}

static int stage_inputs(rovmpc_handle *h, const rovmpc_state *state, const void *U) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_state, state, ROVMPC_STATE_LEN * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_U, U, (size_t)h->cfg.K * h->cfg.N * 3 * h->esz, hipMemcpyHostToDevice, h->stream));
    return ROVMPC_OK;
}

extern "C" int rovmpc_step(rovmpc_handle *h, const rovmpc_state *state, const void *U, double *u_out, double *traj_out,
                           double *best_cost, int64_t *best_idx) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!state || !U) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_step: null state/U");
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = stage_inputs(h, state, U))) return rc;
    if ((rc = enqueue_step(h, h->d_state, h->d_U, h->d_result, h->stream))) return rc;
    const size_t R = rovmpc_result_len(h);
    HIPCHK(h, hipMemcpyAsync(h->h_result, h->d_result, R * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (best_cost) *best_cost = h->h_result[0];
    if (best_idx) *best_idx = (int64_t)h->h_result[1];
    if (u_out) memcpy(u_out, h->h_result + 2, 3 * sizeof(double));
    if (traj_out) memcpy(traj_out, h->h_result + 5, 2 * (size_t)(h->cfg.N + 1) * sizeof(double));
    return ROVMPC_OK;
}

extern "C" int rovmpc_rollout_costs(rovmpc_handle *h, const rovmpc_state *state, const void *U, void *J_out, void *traj_all) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!state || !U || !J_out) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_rollout_costs: null pointer");
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = stage_inputs(h, state, U))) return rc;
    const size_t tbytes = (size_t)h->cfg.K * (h->cfg.N + 1) * 2 * h->esz;
    if (traj_all && !h->d_traj_all) HIPCHK(h, hipMalloc(&h->d_traj_all, tbytes));
    StepOpts o;
    o.traj_all = traj_all ? h->d_traj_all : nullptr;
    if ((rc = enqueue_step(h, h->d_state, h->d_U, nullptr, h->stream, o))) return rc;
    HIPCHK(h, hipMemcpyAsync(J_out, h->d_J, (size_t)h->cfg.K * h->esz, hipMemcpyDeviceToHost, h->stream));
    if (traj_all) HIPCHK(h, hipMemcpyAsync(traj_all, h->d_traj_all, tbytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ROVMPC_OK;
}

// ---- controllers that iterate on a plan (MPPI, CEM): one host path for a single problem and for a batch of B -----------------
// A controller supplies two launches (its sampler and its update) and its sizes (plan_reset); everything else is here.  The
// one-problem controllers (h->mppi, h->cem) are the B = 1 case with `single` set, which the code below asks about in these
// places only: how state and seed reach a step's first sampler (kernel arguments and the one-problem sampler, against the
// mapped staging block and the batched sampler), which update kernel runs (one problem and no step ticket, against
// blockIdx.y = problem and a step ticket, B = 1 included), the buffers (made once, with no device synchronise) and the
// wording of the messages.
static int check_n_iter(rovmpc_handle *h, int n_iter) {
    if (n_iter < 1 || n_iter > 64) FAIL(h, ROVMPC_ERR_INVALID, "n_iter must be in 1..64 (got %d)", n_iter);
    return ROVMPC_OK;
}

static int check_std3(rovmpc_handle *h, const char *name, const double *v) {
    for (int i = 0; i < 3; ++i)
        if (!(isfinite(v[i]) && v[i] >= 0)) FAIL(h, ROVMPC_ERR_INVALID, "%s[%d] must be finite and >= 0 (got %g)", name, i, v[i]);
    return ROVMPC_OK;
}

static int check_single_gpu(rovmpc_handle *h, const char *name) {
    if (h->comm) FAIL(h, ROVMPC_ERR_UNSUPPORTED, "%s is single-GPU: not available once rovmpc_comm_init has run", name);
    return ROVMPC_OK;
}

static const int PLAN_BATCH_MAX = 1024;

static int check_batch_size(rovmpc_handle *h, const char *fn, int B) {
    if (B < 1 || B > PLAN_BATCH_MAX) FAIL(h, ROVMPC_ERR_INVALID, "%s: B must be in 1..%d (got %d)", fn, PLAN_BATCH_MAX, B);
    return ROVMPC_OK;
}

// rovmpc_*_reset and _reset_batch: buffers for B problems (kept when B is the one they were made for, so the single
// controller's are made at its first reset and never again), the plans into half 0 (the spread, where there is one,
// restarts from std at every step)
static int plan_reset(rovmpc_handle *h, PlanCtl &c, int B, const double *plans, size_t slab_words, size_t row_words, bool with_spread) {
    int rc;
    if ((rc = check_single_gpu(h, c.name))) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (B != c.B) {
        PlanCtl fresh{c.name, c.abi, c.single};
        if ((rc = plan_alloc(h, fresh, B, slab_words, row_words, with_spread))) return rc;
        if (B > 1 && (rc = ensure_batch(h, B))) { plan_free(fresh); return rc; }     // the batched rollout's workspace
        if (!c.single) HIPCHK(h, hipDeviceSynchronize());       // nothing may still be using the old buffers (single: there are none)
        plan_free(c);
        c = fresh;
    }
    HIPCHK(h, hipMemcpyAsync(c.plan, plans, (size_t)B * 3 * h->cfg.N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    c.cur = 0;
    return ROVMPC_OK;
}

// rovmpc_*_last and _last_batch: host copies of the last iteration's candidates and costs
static int plan_last(rovmpc_handle *h, PlanCtl &c, void *U_out, void *J_out) {
    if (c.steps == 0) {
        if (c.single) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_%s_last: no %s step yet", c.abi, c.name);
        else FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_%s_last_batch: no batched %s step yet", c.abi, c.name);
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (U_out) HIPCHK(h, hipMemcpy(U_out, c.U, (size_t)c.B * h->cfg.K * h->cfg.N * 3 * h->esz, hipMemcpyDeviceToHost));
    if (J_out) HIPCHK(h, hipMemcpy(J_out, c.J, (size_t)c.B * h->cfg.K * h->esz, hipMemcpyDeviceToHost));
    return ROVMPC_OK;
}

// A device-resident closed loop around the control steps (rovmpc_*_closed_loop*_device): T steps from the measured rows
// d_exo [T][16] ([B][T][16] in a batch), each step's row into d_rows [T][W] ([T][B][W]).  PlanLoop{}: one step from host states.
struct PlanLoop {
    const double *d_exo = nullptr;
    long long T = 1;
    int feedback = 0;
    double *d_rows = nullptr;
    size_t W = 0;
};

// The argument checks the four loop entries share, before anything is launched
static int plan_loop_check(rovmpc_handle *h, const char *fn, const void *d_exo, int64_t T, int32_t feedback, const void *d_rows) {
    if (!d_exo || !d_rows) FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (d_exo or d_rows)", fn);
    if (T < 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: T must be >= 1 (got %lld)", fn, (long long)T);
    if (feedback != 0 && feedback != 1) FAIL(h, ROVMPC_ERR_INVALID, "%s: feedback must be 0 or 1 (got %d)", fn, feedback);
    return ROVMPC_OK;
}

// The checks of a single controller's step that need no parameters (entry: "step" or "closed_loop_device")
static int plan_single_ready(rovmpc_handle *h, PlanCtl &c, const char *entry) {
    int rc;
    if ((rc = check_single_gpu(h, c.name))) return rc;
    if (c.B == 0) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_%s_%s before rovmpc_%s_reset", c.abi, entry, c.abi);
    return ROVMPC_OK;
}

// The same of a batched step (null_arg: one of the entry's required pointers, which `args` names, is null)
static int plan_batch_ready(rovmpc_handle *h, PlanCtl &c, const char *fn, int B, bool null_arg, const char *args) {
    int rc;
    if ((rc = check_batch_size(h, fn, B))) return rc;
    if (null_arg) FAIL(h, ROVMPC_ERR_INVALID, "%s: null pointer (%s)", fn, args);
    if ((rc = check_single_gpu(h, c.name))) return rc;
    if (c.B == 0) FAIL(h, ROVMPC_ERR_INVALID, "%s before rovmpc_%s_reset_batch", fn, c.abi);
    if (B != c.B) FAIL(h, ROVMPC_ERR_INVALID, "%s: B = %d but rovmpc_%s_reset_batch made %d problems", fn, B, c.abi, c.B);
    return ROVMPC_OK;
}

struct ProposalTile { int rows, stride; };

// A tile is `rows` whole candidates, a multiple of 4: about one Philox block per thread (rows 3N <= 1024 elements), one
// phase-2 thread per (row, channel) (3 rows <= PROPOSAL_NT), 4 rows where a row alone is longer.  A tile row takes `stride`
// doubles of LDS, 3N padded up to 3 mod 32 (the bank rule of phase 2): at most 4 x 1027 doubles, 33 KB, per workgroup.
static ProposalTile proposal_tile(int N) {
    const int row3 = 3 * N;
    int rows = 1024 / row3;
    if (rows > PROPOSAL_NT / 3) rows = PROPOSAL_NT / 3;
    rows &= ~3;
    if (rows < 4) rows = 4;
    return {rows, row3 + ((3 - row3 % 32) + 32) % 32};
}

// ---- the navigation cost (nav_kernels.h): C_k of the vehicle's predicted path added to J between rollout and update ----
// One launch for B problems on the tile of the shaped sampler; track_stride: doubles between the problems' tracks.

static int launch_nav_cost(rovmpc_handle *h, const double *d_state, const void *d_U, void *d_J, double *d_C, uint64_t step, int B,
                           size_t track_stride, hipStream_t s) {
    const ProposalTile t = proposal_tile(h->cfg.N);
    NavArgs a;
    memset(&a, 0, sizeof(a));
    a.state = d_state; a.track = h->d_nav_track; a.spheres = h->d_nav_spheres; a.C = d_C;
    a.c = h->cfg.v_scale * h->cfg.dt;
    for (int i = 0; i < 3; ++i) { a.w_pos[i] = h->nav.w_pos[i]; a.w_term[i] = h->nav.w_term[i]; a.w_du[i] = h->nav.w_du[i]; }
    a.w_sphere = h->nav.w_sphere;
    a.K = h->cfg.K; a.Tr = h->nav_Tr; a.r0 = (long long)(step - h->nav.origin); a.track_stride = track_stride;
    a.N = h->cfg.N; a.rows = t.rows; a.stride = t.stride; a.n_spheres = h->nav.n_spheres;
    const dim3 grid((unsigned)((a.K + t.rows - 1) / t.rows), (unsigned)B);
    const size_t lds = (size_t)t.rows * (t.stride + 3) * sizeof(double);
    if (h->cfg.dtype == ROVMPC_F64) hipLaunchKernelGGL(nav_cost_kernel<double>, grid, dim3(NAV_NT), lds, s, a, (const double *)d_U, (double *)d_J);
    else hipLaunchKernelGGL(nav_cost_kernel<float>, grid, dim3(NAV_NT), lds, s, a, (const float *)d_U, (float *)d_J);
    return launched(h, "navigation cost");
}

extern "C" int rovmpc_set_nav_cost(rovmpc_handle *h, const rovmpc_nav_cost *nav, const double *tracks, int32_t Bt, int64_t Tr) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = check_single_gpu(h, "rovmpc_set_nav_cost");
    if (rc) return rc;
    if (!nav) { h->nav_on = false; return ROVMPC_OK; }
    if (nav->struct_size != (int32_t)sizeof(rovmpc_nav_cost))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_nav_cost.struct_size %d != %d (ABI mismatch)", nav->struct_size, (int)sizeof(rovmpc_nav_cost));
    if (nav->n_spheres < 0 || nav->n_spheres > ROVMPC_NAV_MAX_SPHERES)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_nav_cost: n_spheres must be in 0..%d (got %d)", ROVMPC_NAV_MAX_SPHERES, nav->n_spheres);
    if ((rc = check_std3(h, "w_pos", nav->w_pos)) || (rc = check_std3(h, "w_term", nav->w_term)) || (rc = check_std3(h, "w_du", nav->w_du))) return rc;
    if (!(isfinite(nav->w_sphere) && nav->w_sphere >= 0)) FAIL(h, ROVMPC_ERR_INVALID, "w_sphere must be finite and >= 0 (got %g)", nav->w_sphere);
    for (int j = 0; j < nav->n_spheres; ++j) {
        const double *sp = nav->spheres[j];
        if (!(isfinite(sp[0]) && isfinite(sp[1]) && isfinite(sp[2]) && isfinite(sp[3]) && sp[3] >= 0))
            FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_nav_cost: sphere %d must be finite with R >= 0 (got %g, %g, %g, %g)", j, sp[0], sp[1], sp[2], sp[3]);
    }
    if (!tracks) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_nav_cost: null tracks");
    if (Bt < 1 || Tr < 1 || Tr > (1 << 24) || (long long)Bt * Tr > (1 << 24))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_nav_cost: need Bt >= 1, Tr >= 1 and Bt * Tr <= %d (got %d, %lld)", 1 << 24, Bt, (long long)Tr);
    const size_t n = (size_t)Bt * (size_t)Tr * 3;
    for (size_t i = 0; i < n; ++i)
        if (!isfinite(tracks[i])) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_nav_cost: tracks[%zu][%zu][%zu] is not finite", i / (3 * (size_t)Tr), i / 3 % (size_t)Tr, i % 3);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));             // no step of the handle is reading the buffers about to change
    if (!h->d_nav_spheres) HIPCHK(h, hipMalloc((void **)&h->d_nav_spheres, sizeof(nav->spheres)));
    if (n > h->nav_track_cap) {
        double *fresh = nullptr;
        HIPCHK(h, hipMalloc((void **)&fresh, n * sizeof(double)));
        dev_free(h->d_nav_track);
        h->d_nav_track = fresh; h->nav_track_cap = n;
        h->nav_on = false;                                  // until the copies below have succeeded
    }
    hipError_t e = hipMemcpy(h->d_nav_track, tracks, n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_nav_spheres, nav->spheres, sizeof(nav->spheres), hipMemcpyHostToDevice);
    if (e != hipSuccess) { h->nav_on = false; FAIL(h, ROVMPC_ERR_HIP, "rovmpc_set_nav_cost: copying the tracks: %s", hipGetErrorString(e)); }
    h->nav = *nav; h->nav_Bt = Bt; h->nav_Tr = Tr; h->nav_on = true;
    return ROVMPC_OK;
}

extern "C" int rovmpc_nav_cost_device(rovmpc_handle *h, const double *d_state, const void *d_U, uint64_t step, double *d_C, void *d_J,
                                      void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = check_single_gpu(h, "rovmpc_nav_cost_device");
    if (rc) return rc;
    if (!h->nav_on) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_nav_cost_device: no navigation cost is set (rovmpc_set_nav_cost)");
    if (!d_state || !d_U) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_nav_cost_device: null pointer (d_state or d_U)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return launch_nav_cost(h, d_state, d_U, d_J, d_C, step, 1, 0, (hipStream_t)stream);
}

// ---- the tether keep-out cost (tether_kernels.h): C_k of the cable's predicted shapes added to J after the navigation cost ----
// The tile: TETHER_ROWS candidates with the LDS row stride of the shaped sampler, and as many nodes per chunk as fit into
// 64 KB beside it (0: not even one).
static int tether_chunk(const rovmpc_config &c, size_t *lds_out) {
    const ProposalTile t = proposal_tile(c.N);
    const size_t tile = (size_t)TETHER_ROWS * t.stride * sizeof(double);
    const size_t node = (size_t)TETHER_ROWS * (TETHER_PAR + 3 * (size_t)c.n_shape_pts) * sizeof(double);
    if (tile + node > 64 * 1024) return 0;
    size_t nc = (64 * 1024 - tile) / node;
    if (nc > (size_t)c.N) nc = (size_t)c.N;
    if (lds_out) *lds_out = tile + nc * node;
    return (int)nc;
}

static int launch_tether_cost(rovmpc_handle *h, const double *d_state, const void *d_U, const void *d_traj, void *d_J, double *d_C,
                              double *d_D, int B, hipStream_t s) {
    const rovmpc_config &c = h->cfg;
    const bool f64 = c.dtype == ROVMPC_F64;
    size_t lds = 0;
    TetherArgs a;
    memset(&a, 0, sizeof(a));
    a.state = d_state; a.spheres = h->d_tether_spheres; a.C = d_C; a.D = d_D;
    a.c = c.v_scale * c.dt;
    a.w = h->tether.w; a.margin = h->tether.margin;
    a.L = f64 ? c.L : (double)(float)c.L; a.c_lo = f64 ? c.c_lo : (double)(float)c.c_lo; a.c_hi = f64 ? c.c_hi : (double)(float)c.c_hi;
    a.up = c.frame == ROVMPC_ENU ? 1.0 : -1.0;
    a.K = c.K; a.N = c.N; a.M = c.n_shape_pts; a.rows = TETHER_ROWS; a.stride = proposal_tile(c.N).stride;
    a.nc = tether_chunk(c, &lds); a.n_spheres = h->tether.n_spheres;
    const dim3 grid((unsigned)((a.K + a.rows - 1) / a.rows), (unsigned)B);
    if (f64) hipLaunchKernelGGL(tether_cost_kernel<double>, grid, dim3(TETHER_NT), lds, s, a, (const double *)d_U, (const double *)d_traj, (double *)d_J);
    else hipLaunchKernelGGL(tether_cost_kernel<float>, grid, dim3(TETHER_NT), lds, s, a, (const float *)d_U, (const float *)d_traj, (float *)d_J);
    return launched(h, "tether cost");
}

// the trajectory buffer for B problems; a larger one is made before the old one is let go
static int ensure_tether_traj(rovmpc_handle *h, int B) {
    if (B <= h->tether_cap) return ROVMPC_OK;
    void *fresh = nullptr;
    hipError_t e = hipMalloc(&fresh, (size_t)B * h->cfg.K * (h->cfg.N + 1) * 2 * h->esz);
    if (e == hipSuccess) e = hipDeviceSynchronize();        // nothing may still be using the old buffer
    if (e != hipSuccess) {
        if (fresh) (void)hipFree(fresh);
        (void)hipGetLastError();
        FAIL(h, ROVMPC_ERR_HIP, "tether cost: trajectory buffer for %d problems: %s", B, hipGetErrorString(e));
    }
    dev_free(h->d_tether_traj);
    h->d_tether_traj = fresh; h->tether_cap = B;
    return ROVMPC_OK;
}

extern "C" int rovmpc_set_tether_cost(rovmpc_handle *h, const rovmpc_tether_cost *tc) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = check_single_gpu(h, "rovmpc_set_tether_cost");
    if (rc) return rc;
    if (!tc) { h->tether_on = false; return ROVMPC_OK; }
    if (tc->struct_size != (int32_t)sizeof(rovmpc_tether_cost))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_tether_cost.struct_size %d != %d (ABI mismatch)", tc->struct_size, (int)sizeof(rovmpc_tether_cost));
    if (tc->n_spheres < 1 || tc->n_spheres > ROVMPC_TETHER_MAX_SPHERES)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_tether_cost: n_spheres must be in 1..%d (got %d)", ROVMPC_TETHER_MAX_SPHERES, tc->n_spheres);
    if (!(isfinite(tc->w) && tc->w >= 0)) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_tether_cost: w must be finite and >= 0 (got %g)", tc->w);
    if (!(isfinite(tc->margin) && tc->margin >= 0)) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_tether_cost: margin must be finite and >= 0 (got %g)", tc->margin);
    for (int j = 0; j < tc->n_spheres; ++j) {
        const double *sp = tc->spheres[j];
        if (!(isfinite(sp[0]) && isfinite(sp[1]) && isfinite(sp[2]) && isfinite(sp[3]) && sp[3] >= 0))
            FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_tether_cost: sphere %d must be finite with R >= 0 (got %g, %g, %g, %g)", j, sp[0], sp[1], sp[2], sp[3]);
    }
    if (tether_chunk(h->cfg, nullptr) < 1)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_tether_cost: N = %d with n_shape_pts = %d does not leave room for one node in 64 KB of LDS", h->cfg.N, h->cfg.n_shape_pts);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));             // no step of the handle is reading the spheres about to change
    int B = 1;
    for (const PlanCtl *c : {&h->mppi_b, &h->cem_b}) if (c->B > B) B = c->B;
    if ((rc = ensure_tether_traj(h, B))) return rc;
    if (!h->d_tether_spheres) HIPCHK(h, hipMalloc((void **)&h->d_tether_spheres, sizeof(tc->spheres)));
    hipError_t e = hipMemcpy(h->d_tether_spheres, tc->spheres, sizeof(tc->spheres), hipMemcpyHostToDevice);
    if (e != hipSuccess) { h->tether_on = false; FAIL(h, ROVMPC_ERR_HIP, "rovmpc_set_tether_cost: copying the spheres: %s", hipGetErrorString(e)); }
    h->tether = *tc; h->tether_on = true;
    return ROVMPC_OK;
}

extern "C" int rovmpc_tether_cost_device(rovmpc_handle *h, const double *d_state, const void *d_U, const void *d_traj, double *d_C,
                                         double *d_D, void *d_J, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = check_single_gpu(h, "rovmpc_tether_cost_device");
    if (rc) return rc;
    if (!h->tether_on) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_tether_cost_device: no tether cost is set (rovmpc_set_tether_cost)");
    if (!d_state || !d_U || !d_traj) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_tether_cost_device: null pointer (d_state, d_U or d_traj)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return launch_tether_cost(h, d_state, d_U, d_traj, d_J, d_C, d_D, 1, (hipStream_t)stream);
}

// What the loop hands the two launches of iteration i.  The last group is set in the last iteration of a step only (the
// update then also shifts the plan by one node, passes the rollout's record on and, where the step has a mailbox, fills
// it); *_update_device passes PlanIter{}.
struct PlanIter {
    bool first = false;                    // iteration 0 of its step (CEM: the spread restarts from std)
    // How state and seed reach the sampler.  Single: as kernel arguments, the state in the call's first iteration only
    // (from the host, or in a loop from device memory); the sampler stores it for the step's rollouts.
    uint64_t seed = 0;
    const rovmpc_state *state = nullptr;
    const double *state_src = nullptr;
    PlanBatchIn in = {};                   // batched: the staging block, in the call's first iteration only
    uint64_t counter = 0;                  // of the draw: step * n_iter + i (wraps)
    size_t in_off = 0, out_off = 0;        // offsets of the halves of plan (and spread) the iteration reads and writes: [B][3N] each
    int shift = 0;
    double *record = nullptr, *host_out = nullptr;     // host_out, done_flag: a single step, or the last step of a loop
    unsigned long long *done_flag = nullptr, done_seq = 0;
    PlanHandoff loop = {};                 // a loop's steps: the rows in device memory and the next step's states
};

// All eight step and loop entries: seeds (and, for a step, states) of a batch into the staging block, then
// loop.T x n_iter x (sample, rollout, update) on the handle's stream without a host round trip, then one wait for the
// mailbox, which the last step's last update fills.  sample(it) and update(it) launch the controller's kernels.  In a loop
// (states null) the first sampler takes the states from row 0 of each problem's exo trajectory and every later step finds
// them where its predecessor left them.
template <typename Sample, typename Update>
static int plan_step(rovmpc_handle *h, PlanCtl &c, const rovmpc_state *states, const PlanLoop &loop, const uint64_t *seeds,
                     uint64_t step, int n_iter, Sample sample, Update update) {
    int rc;
    if ((rc = check_ready(h))) return rc;
    if (h->nav_on && !c.single && h->nav_Bt != 1 && h->nav_Bt != c.B)
        FAIL(h, ROVMPC_ERR_INVALID, "batched %s: B = %d but the navigation cost has %d tracks (rovmpc_set_nav_cost: one per problem, or one for all)",
             c.name, c.B, h->nav_Bt);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (c.B > 1 && (rc = ensure_batch(h, c.B))) return rc;     // an early-out unless a failed growth elsewhere took it away
    if (h->tether_on && (rc = ensure_tether_traj(h, c.B))) return rc;      // the batch grew after the setting was made
    void *const traj_all = h->tether_on ? h->d_tether_traj : nullptr;
    StepOpts rollout;                            // the rollouts write the controller's own costs, not the handle's
    rollout.J = c.J; rollout.traj_all = traj_all; rollout.B = c.B;
    const size_t B = (size_t)c.B, half = B * 3 * (size_t)h->cfg.N, exo_stride = (size_t)loop.T * ROVMPC_STATE_LEN;
    if (!c.single) {
        if (states) memcpy(c.h_stage, states, B * sizeof(rovmpc_state));
        memcpy(c.h_stage + B * ROVMPC_STATE_LEN, seeds, B * sizeof(uint64_t));
    }
    const unsigned long long seq = ++c.box.seq;
    int cur = c.cur;
    for (long long t = 0; t < loop.T; ++t) {
        const bool last_step = t + 1 == loop.T;
        for (int i = 0; i < n_iter; ++i) {
            const bool start = i == 0 && t == 0;
            PlanIter it;
            it.first = i == 0;
            if (!c.single) it.in = PlanBatchIn{start ? c.d_stage : nullptr, c.state, c.seeds, c.B, loop.d_exo, exo_stride};
            else { it.seed = *seeds; if (start) { it.state = states; it.state_src = loop.d_exo; } }
            it.counter = (step + (uint64_t)t) * (uint64_t)n_iter + (uint64_t)i;
            // (done_seq is read only where done_flag is set, and the strides of `loop` only for problems b > 0: a single
            // controller's launches carry them too, where the two separate paths left zeros)
            it.in_off = cur * half; it.out_off = (cur ^ 1) * half; it.done_seq = seq;
            if (i + 1 == n_iter) {
                it.shift = 1; it.record = c.record;
                if (last_step) { it.host_out = c.box.d_out; it.done_flag = c.box.d_done; }
                if (loop.d_rows)
                    it.loop = PlanHandoff{loop.d_rows + (size_t)t * B * loop.W, last_step ? nullptr : loop.d_exo + (size_t)(t + 1) * ROVMPC_STATE_LEN,
                                          c.state, loop.feedback, loop.W, exo_stride};
            }
            if ((rc = sample(it))) return rc;
            if ((rc = enqueue_step(h, c.state, c.U, c.record, h->stream, rollout))) return rc;
            if (h->nav_on && (rc = launch_nav_cost(h, c.state, c.U, c.J, nullptr, step + (uint64_t)t, c.B,
                                                   !c.single && h->nav_Bt == c.B ? 3 * (size_t)h->nav_Tr : 0, h->stream))) return rc;
            if (traj_all && (rc = launch_tether_cost(h, c.state, c.U, traj_all, c.J, nullptr, nullptr, c.B, h->stream))) return rc;
            if ((rc = update(it))) return rc;
            cur ^= 1;
        }
    }
    c.cur = cur;
    c.steps += (unsigned long long)loop.T;
    return mailbox_wait(h, c.box, seq, c.single ? (std::string(c.name) + " step").c_str() : c.name);      // (the wording of each form's message)
}

// state and seed of a single controller's sampler: kernel arguments
template <typename SA> static void plan_single_in(SA &sa, const PlanCtl &c, const PlanIter &it) {
    sa.seed = it.seed;
    if (it.state) sa.state = *it.state;
    sa.state_src = it.state_src;
    if (it.state || it.state_src) sa.d_state = c.state;
}

// an update's arguments for the B problems of c (blockIdx.y = problem); only a step with a mailbox takes the step ticket
template <typename BA, typename A> static BA plan_batch_args(const A &a, const PlanCtl &c) {
    BA ba;
    memset(&ba, 0, sizeof(ba));
    ba.a = a; ba.slab_stride = c.slab_stride; ba.host_stride = c.row; ba.B = c.B;
    if (a.host_out) ba.step_ticket = c.tickets + c.B;
    return ba;
}

#define LAUNCH_SAMPLER(kern, h, grid, sa, U)                                                                                  \
    do {                                                                                                                      \
        if ((h)->cfg.dtype == ROVMPC_F64) hipLaunchKernelGGL(kern<double>, grid, dim3(SAMPLER_NT), 0, (h)->stream, sa, (double *)(U)); \
        else hipLaunchKernelGGL(kern<float>, grid, dim3(SAMPLER_NT), 0, (h)->stream, sa, (float *)(U));                       \
    } while (0)

// ---- the shaped proposal (proposal_kernels.h): AR(1) noise along the horizon and a box, for MPPI and CEM alike --------
// The draw around `mean` with spread `sigma` (null: std3 on every node) inside [lo3, hi3], for c's problems
static int launch_proposal_sample(rovmpc_handle *h, const PlanCtl &c, const PlanIter &it, const double *std3, const double *lo3,
                                  const double *hi3, const double *mean, const double *sigma, const char *what) {
    const ProposalTile t = proposal_tile(h->cfg.N);
    ProposalLaw law;
    memset(&law, 0, sizeof(law));
    law.counter = it.counter;
    for (int i = 0; i < 3; ++i) {
        law.beta[i] = h->prop_beta[i]; law.root[i] = h->prop_root[i]; law.std[i] = std3[i]; law.lo[i] = lo3[i]; law.hi[i] = hi3[i];
    }
    law.K = h->cfg.K; law.N = h->cfg.N; law.rows = t.rows; law.stride = t.stride; law.mean = mean; law.sigma = sigma;
    const int gx = (int)((law.K + t.rows - 1) / t.rows);
    const size_t lds = (size_t)t.rows * t.stride * sizeof(double);
    const bool f64 = h->cfg.dtype == ROVMPC_F64;
    if (c.single) {
        ProposalSampleArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.law = law;
        plan_single_in(sa, c, it);
        if (f64) hipLaunchKernelGGL(proposal_sample_kernel<double>, dim3(gx), dim3(PROPOSAL_NT), lds, h->stream, sa, (double *)c.U);
        else hipLaunchKernelGGL(proposal_sample_kernel<float>, dim3(gx), dim3(PROPOSAL_NT), lds, h->stream, sa, (float *)c.U);
        return launched(h, what);
    }
    ProposalSampleBatchArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.law = law; sa.in = it.in;
    if (f64) hipLaunchKernelGGL(proposal_sample_batch_kernel<double>, dim3(gx, c.B), dim3(PROPOSAL_NT), lds, h->stream, sa, (double *)c.U);
    else hipLaunchKernelGGL(proposal_sample_batch_kernel<float>, dim3(gx, c.B), dim3(PROPOSAL_NT), lds, h->stream, sa, (float *)c.U);
    return launched(h, what);
}

extern "C" int rovmpc_set_noise_correlation(rovmpc_handle *h, const double *beta3) {
    if (!h) return ROVMPC_ERR_INVALID;
    const double zero[3] = {0.0, 0.0, 0.0};
    if (!beta3) beta3 = zero;
    for (int i = 0; i < 3; ++i)
        if (!(isfinite(beta3[i]) && beta3[i] >= 0 && beta3[i] < 1))
            FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_set_noise_correlation: beta[%d] must be finite and in [0, 1) (got %g)", i, beta3[i]);
    h->prop_colored = false;
    for (int i = 0; i < 3; ++i) {
        h->prop_beta[i] = beta3[i];
        h->prop_root[i] = sqrt((1.0 - beta3[i]) * (1.0 + beta3[i]));
        if (beta3[i] != 0) h->prop_colored = true;
    }
    return ROVMPC_OK;
}

extern "C" int rovmpc_mppi_set_bounds(rovmpc_handle *h, const double *lo3, const double *hi3) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!lo3 != !hi3) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_set_bounds: lo and hi must both be given or both be null");
    for (int i = 0; lo3 && i < 3; ++i)
        if (!(lo3[i] <= hi3[i])) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_set_bounds: need lo[%d] <= hi[%d], not NaN (got %g, %g)", i, i, lo3[i], hi3[i]);
    h->mppi_boxed = false;
    for (int i = 0; i < 3; ++i) {
        h->mppi_lo[i] = lo3 ? lo3[i] : -INFINITY;
        h->mppi_hi[i] = hi3 ? hi3[i] : INFINITY;
        if (h->mppi_lo[i] != -INFINITY || h->mppi_hi[i] != INFINITY) h->mppi_boxed = true;
    }
    return ROVMPC_OK;
}

// ---- MPPI: sampling around a warm-started nominal, exp(-J/lambda)-weighted update on the GPU -------------------------
struct MppiGeo { int G; long long slice; };
static MppiGeo mppi_geometry(long long K) {
    long long G = (K + MPPI_ROWS_PER_WG - 1) / MPPI_ROWS_PER_WG;
    if (G > MPPI_MAX_WG) G = MPPI_MAX_WG;
    const long long slice = (K + G - 1) / G;
    return {(int)((K + slice - 1) / slice), slice};
}

static int mppi_check_params(rovmpc_handle *h, const rovmpc_mppi_params *p) {
    if (!p) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_step: null params");
    if (p->struct_size != (int32_t)sizeof(rovmpc_mppi_params))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_params.struct_size %d != %d (ABI mismatch)", p->struct_size, (int)sizeof(rovmpc_mppi_params));
    int rc = check_n_iter(h, p->n_iter);
    if (rc) return rc;
    if (!(isfinite(p->lambda) && p->lambda > 0)) FAIL(h, ROVMPC_ERR_INVALID, "lambda must be finite and > 0 (got %g)", p->lambda);
    return check_std3(h, "std", p->std);
}

// slab [G][3 + 3N]
static size_t mppi_slab_bytes(const rovmpc_handle *h) {
    return (size_t)mppi_geometry(h->cfg.K).G * (3 + 3 * (size_t)h->cfg.N) * sizeof(double);
}

// row of a control step: record, nu* (3N), stats (4) -- the mailbox row of a problem too
static size_t mppi_row_words(const rovmpc_handle *h) { return (size_t)rovmpc_result_len(h) + 3 * (size_t)h->cfg.N + 4; }

extern "C" int32_t rovmpc_mppi_row_len(const rovmpc_handle *h) { return h ? (int32_t)mppi_row_words(h) : 0; }

// The update's launch on problem 0's pointers: one problem (batch null: a single controller, rovmpc_mppi_update_device), or
// the B problems of *batch.  pub: the iteration's publish fields.
static int launch_mppi_update(rovmpc_handle *h, const void *d_J, const void *d_U, double lambda, const double *nu_in, double *nu_out,
                              double *stats, void *slab, unsigned *ticket, const PlanIter &pub, const PlanCtl *batch, hipStream_t s) {
    const MppiGeo g = mppi_geometry(h->cfg.K);
    MppiUpdateArgs a;
    memset(&a, 0, sizeof(a));
    a.J = d_J; a.U = d_U; a.K = h->cfg.K; a.slice = g.slice; a.C3 = 3 * h->cfg.N; a.G = g.G; a.lambda = lambda;
    a.nu_in = nu_in; a.nu_out = nu_out; a.shift = pub.shift; a.stats = stats; a.slab = (double *)slab; a.ticket = ticket;
    a.record = pub.record; a.R = rovmpc_result_len(h); a.host_out = pub.host_out; a.done_flag = pub.done_flag; a.done_seq = pub.done_seq;
    a.loop = pub.loop;
    for (int i = 0; i < 3; ++i) { a.lo[i] = h->mppi_lo[i]; a.hi[i] = h->mppi_hi[i]; }
    if (!batch) {
        if (h->mppi_boxed) LAUNCH_T_QC(mppi_update_box_kernel, h, a.C3 > MPPI_NT, dim3(g.G), dim3(MPPI_NT), 0, s, a);
        else LAUNCH_T_QC(mppi_update_kernel, h, a.C3 > MPPI_NT, dim3(g.G), dim3(MPPI_NT), 0, s, a);
        return launched(h, "MPPI update");
    }
    const MppiUpdateBatchArgs ba = plan_batch_args<MppiUpdateBatchArgs>(a, *batch);
    if (h->mppi_boxed) LAUNCH_T_QC(mppi_update_box_batch_kernel, h, a.C3 > MPPI_NT, dim3(g.G, batch->B), dim3(MPPI_NT), 0, s, ba);
    else LAUNCH_T_QC(mppi_update_batch_kernel, h, a.C3 > MPPI_NT, dim3(g.G, batch->B), dim3(MPPI_NT), 0, s, ba);
    return launched(h, "batched MPPI update");
}

template <typename SA> static SA mppi_sample_args(const rovmpc_handle *h, const PlanIter &it, const double *std3, const double *nu) {
    SA sa;
    memset(&sa, 0, sizeof(sa));
    sa.counter = it.counter;
    for (int i = 0; i < 3; ++i) sa.std[i] = std3[i];
    sa.total = (long long)h->cfg.K * h->cfg.N * 3; sa.N = h->cfg.N; sa.nu = nu;
    return sa;
}

static int launch_mppi_sample(rovmpc_handle *h, const PlanCtl &c, const PlanIter &it, const double *std3) {
    const double *nu = c.plan + it.in_off;
    if (h->prop_colored || h->mppi_boxed)
        return launch_proposal_sample(h, c, it, std3, h->mppi_lo, h->mppi_hi, nu, nullptr, c.single ? "MPPI sampler" : "batched MPPI sampler");
    const int gx = sampler_grid((long long)h->cfg.K * h->cfg.N * 3);
    if (c.single) {
        MppiSampleArgs sa = mppi_sample_args<MppiSampleArgs>(h, it, std3, nu);
        plan_single_in(sa, c, it);
        LAUNCH_SAMPLER(mppi_sample_kernel, h, dim3(gx), sa, c.U);
        return launched(h, "MPPI sampler");
    }
    MppiSampleBatchArgs sa = mppi_sample_args<MppiSampleBatchArgs>(h, it, std3, nu);
    sa.in = it.in;
    LAUNCH_SAMPLER(mppi_sample_batch_kernel, h, dim3(gx, c.B), sa, c.U);
    return launched(h, "batched MPPI sampler");
}

// one step of c's problems from host states, or a device loop of loop.T steps; then the mailbox rows into the caller's arrays
static int mppi_run(rovmpc_handle *h, PlanCtl &c, const rovmpc_state *states, const PlanLoop &loop, const uint64_t *seeds, uint64_t step,
                    const rovmpc_mppi_params *p, double *records_out = nullptr, double *nominals_out = nullptr, double *stats_out = nullptr) {
    int rc = plan_step(h, c, states, loop, seeds, step, p->n_iter,
                       [&](const PlanIter &it) { return launch_mppi_sample(h, c, it, p->std); },
                       [&](const PlanIter &it) {
                           return launch_mppi_update(h, c.J, c.U, p->lambda, c.plan + it.in_off, c.plan + it.out_off, nullptr, c.slab,
                                                     c.tickets, it, c.single ? nullptr : &c, h->stream);
                       });
    if (rc) return rc;
    const size_t C3 = 3 * (size_t)h->cfg.N, R = (size_t)rovmpc_result_len(h);
    for (size_t b = 0; records_out && b < (size_t)c.B; ++b) {
        const double *o = c.box.h_out + b * c.row;
        memcpy(records_out + b * R, o, R * sizeof(double));
        if (nominals_out) memcpy(nominals_out + b * C3, o + R, C3 * sizeof(double));
        if (stats_out) memcpy(stats_out + b * 4, o + R + C3, 4 * sizeof(double));
    }
    return take_device_errors(h);
}

extern "C" int rovmpc_mppi_reset(rovmpc_handle *h, const double *nominal) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!nominal) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_reset: null nominal");
    return plan_reset(h, h->mppi, 1, nominal, mppi_slab_bytes(h) / 8, mppi_row_words(h), false);
}

extern "C" int rovmpc_mppi_step(rovmpc_handle *h, const rovmpc_state *state, uint64_t seed, uint64_t step,
                                const rovmpc_mppi_params *p, double *record_out, double *nominal_out, double *stats_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!state || !record_out) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_step: null pointer");
    int rc = mppi_check_params(h, p);
    if (rc || (rc = plan_single_ready(h, h->mppi, "step"))) return rc;
    return mppi_run(h, h->mppi, state, PlanLoop{}, &seed, step, p, record_out, nominal_out, stats_out);
}

extern "C" int rovmpc_mppi_closed_loop_device(rovmpc_handle *h, const double *d_exo, int64_t T, int32_t feedback, uint64_t seed,
                                              uint64_t step0, const rovmpc_mppi_params *p, double *d_rows) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = plan_loop_check(h, "rovmpc_mppi_closed_loop_device", d_exo, T, feedback, d_rows);
    if (rc || (rc = mppi_check_params(h, p)) || (rc = plan_single_ready(h, h->mppi, "closed_loop_device"))) return rc;
    return mppi_run(h, h->mppi, nullptr, PlanLoop{d_exo, T, feedback, d_rows, mppi_row_words(h)}, &seed, step0, p);
}

extern "C" int rovmpc_mppi_last(rovmpc_handle *h, void *U_out, void *J_out) {
    return h ? plan_last(h, h->mppi, U_out, J_out) : ROVMPC_ERR_INVALID;
}

extern "C" int rovmpc_mppi_update_device(rovmpc_handle *h, const void *d_J, const void *d_U, double lambda,
                                         const double *d_nominal_in, double *d_nominal_out, double *d_stats, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!d_J || !d_U || !d_nominal_in || !d_nominal_out) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_update_device: null pointer");
    if (!(isfinite(lambda) && lambda > 0)) FAIL(h, ROVMPC_ERR_INVALID, "lambda must be finite and > 0 (got %g)", lambda);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Slab &x = h->mppi_slab_x;
    int rc = slab_alloc(h, x, mppi_slab_bytes(h));
    if (rc) return rc;
    return launch_mppi_update(h, d_J, d_U, lambda, d_nominal_in, d_nominal_out, d_stats, x.rows, x.ticket, PlanIter{}, nullptr, (hipStream_t)stream);
}

extern "C" int rovmpc_mppi_reset_batch(rovmpc_handle *h, int32_t B, const double *nominals) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = check_batch_size(h, "rovmpc_mppi_reset_batch", B);
    if (rc) return rc;
    if (!nominals) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_mppi_reset_batch: null nominals");
    return plan_reset(h, h->mppi_b, B, nominals, mppi_slab_bytes(h) / 8, mppi_row_words(h), false);
}

extern "C" int rovmpc_mppi_step_batch(rovmpc_handle *h, int32_t B, const rovmpc_state *states, const uint64_t *seeds, uint64_t step,
                                      const rovmpc_mppi_params *p, double *records_out, double *nominals_out, double *stats_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = plan_batch_ready(h, h->mppi_b, "rovmpc_mppi_step_batch", B, !states || !seeds || !records_out, "states, seeds or records_out");
    if (rc || (rc = mppi_check_params(h, p))) return rc;
    return mppi_run(h, h->mppi_b, states, PlanLoop{}, seeds, step, p, records_out, nominals_out, stats_out);
}

extern "C" int rovmpc_mppi_closed_loop_batch_device(rovmpc_handle *h, int32_t B, const double *d_exo, int64_t T, int32_t feedback,
                                                    const uint64_t *seeds, uint64_t step0, const rovmpc_mppi_params *p, double *d_rows) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = plan_batch_ready(h, h->mppi_b, "rovmpc_mppi_closed_loop_batch_device", B, !d_exo || !seeds || !d_rows, "d_exo, seeds or d_rows");
    if (rc || (rc = plan_loop_check(h, "rovmpc_mppi_closed_loop_batch_device", d_exo, T, feedback, d_rows)) || (rc = mppi_check_params(h, p))) return rc;
    return mppi_run(h, h->mppi_b, nullptr, PlanLoop{d_exo, T, feedback, d_rows, mppi_row_words(h)}, seeds, step0, p);
}

extern "C" int rovmpc_mppi_last_batch(rovmpc_handle *h, void *U_out, void *J_out) {
    return h ? plan_last(h, h->mppi_b, U_out, J_out) : ROVMPC_ERR_INVALID;
}

// ---- CEM: clamped sampling around a per-node mean and spread, exact elite selection and refit on the GPU ---------------
struct CemGeo { int G; long long slice; int Lcap; };
static CemGeo cem_geometry(long long K) {
    const long long G = (K + CEM_SLICE - 1) / CEM_SLICE, slice = (K + G - 1) / G;
    return {(int)((K + slice - 1) / slice), slice, (int)(slice < CEM_MAX_ELITE ? slice : CEM_MAX_ELITE)};
}

static int cem_check_params(rovmpc_handle *h, const rovmpc_cem_params *p) {
    if (!p) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_cem: null params");
    if (p->struct_size != (int32_t)sizeof(rovmpc_cem_params))
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_cem_params.struct_size %d != %d (ABI mismatch)", p->struct_size, (int)sizeof(rovmpc_cem_params));
    int rc = check_n_iter(h, p->n_iter);
    if (rc) return rc;
    const int emax = h->cfg.K < CEM_MAX_ELITE ? h->cfg.K : CEM_MAX_ELITE;
    if (p->n_elite < 1 || p->n_elite > emax) FAIL(h, ROVMPC_ERR_INVALID, "n_elite must be in 1..%d = min(K, %d) (got %d)", emax, CEM_MAX_ELITE, p->n_elite);
    if (p->reserved != 0) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_cem_params.reserved must be 0 (got %d)", p->reserved);
    if (!(isfinite(p->alpha) && p->alpha >= 0 && p->alpha < 1)) FAIL(h, ROVMPC_ERR_INVALID, "alpha must be finite, 0 <= alpha < 1 (got %g)", p->alpha);
    if ((rc = check_std3(h, "std", p->std)) || (rc = check_std3(h, "std_min", p->std_min))) return rc;
    for (int i = 0; i < 3; ++i)
        if (isnan(p->lo[i]) || isnan(p->hi[i]) || !(p->lo[i] <= p->hi[i]))
            FAIL(h, ROVMPC_ERR_INVALID, "bounds of channel %d must not be NaN and lo <= hi (got %g, %g)", i, p->lo[i], p->hi[i]);
    return ROVMPC_OK;
}

// slab [G][2 + 2 Lcap], only when the update has several workgroups
static size_t cem_slab_bytes(const rovmpc_handle *h) {
    const CemGeo g = cem_geometry(h->cfg.K);
    return g.G > 1 ? (size_t)g.G * (2 + 2 * (size_t)g.Lcap) * sizeof(unsigned long long) : 0;
}

// mailbox row of a problem: record, mu* (3N), sigma* (3N), stats (4), then the elite list (int64 [CEM_MAX_ELITE])
static size_t cem_row_words(const rovmpc_handle *h) { return (size_t)rovmpc_result_len(h) + 6 * (size_t)h->cfg.N + 4 + CEM_MAX_ELITE; }

// row of a loop's control step: record, mu* (3N), sigma* (3N), stats (4), the elite list (n_elite, int64)
static size_t cem_loop_row_words(const rovmpc_handle *h, int n_elite) { return (size_t)rovmpc_result_len(h) + 6 * (size_t)h->cfg.N + 4 + (size_t)n_elite; }

extern "C" int32_t rovmpc_cem_row_len(const rovmpc_handle *h, int32_t n_elite) {
    return h && n_elite >= 1 && n_elite <= CEM_MAX_ELITE ? (int32_t)cem_loop_row_words(h, n_elite) : 0;
}

// The update's launch on problem 0's pointers: one problem (batch null: a single controller, rovmpc_cem_update_device), or
// the B problems of *batch.  pub: the iteration's publish fields; the elite list of a mailbox row lies behind its stats.
static int launch_cem_update(rovmpc_handle *h, const void *d_J, const void *d_U, const rovmpc_cem_params *p, const double *mu_in,
                             const double *sigma_in, double *mu_out, double *sigma_out, long long *elite, double *stats,
                             void *slab, unsigned *ticket, const PlanIter &pub, const PlanCtl *batch, hipStream_t s) {
    const CemGeo g = cem_geometry(h->cfg.K);
    CemUpdateArgs a;
    memset(&a, 0, sizeof(a));
    a.J = d_J; a.U = d_U; a.K = h->cfg.K; a.slice = g.slice; a.C3 = 3 * h->cfg.N; a.G = g.G; a.E = p->n_elite; a.Lcap = g.Lcap;
    a.alpha = p->alpha;
    for (int i = 0; i < 3; ++i) { a.std[i] = p->std[i]; a.std_min[i] = p->std_min[i]; a.lo[i] = p->lo[i]; a.hi[i] = p->hi[i]; }
    a.mu_in = mu_in; a.sigma_in = sigma_in; a.mu_out = mu_out; a.sigma_out = sigma_out; a.shift = pub.shift;
    a.elite = elite; a.stats = stats; a.slab = (unsigned long long *)slab; a.ticket = ticket;
    a.record = pub.record; a.R = rovmpc_result_len(h); a.host_out = pub.host_out;
    if (pub.host_out) a.host_elite = (long long *)(pub.host_out + a.R + 2 * a.C3 + 4);
    a.done_flag = pub.done_flag; a.done_seq = pub.done_seq;
    a.loop = pub.loop;
    if (!batch) {
        LAUNCH_T_QC(cem_update_kernel, h, a.C3 > CEM_NT, dim3(g.G), dim3(CEM_NT), 0, s, a);
        return launched(h, "CEM update");
    }
    const CemUpdateBatchArgs ba = plan_batch_args<CemUpdateBatchArgs>(a, *batch);
    LAUNCH_T_QC(cem_update_batch_kernel, h, a.C3 > CEM_NT, dim3(g.G, batch->B), dim3(CEM_NT), 0, s, ba);
    return launched(h, "batched CEM update");
}

template <typename SA> static SA cem_sample_args(const rovmpc_handle *h, const PlanIter &it, const rovmpc_cem_params *p, const double *mu,
                                                 const double *sigma) {
    SA sa;
    memset(&sa, 0, sizeof(sa));
    sa.counter = it.counter;
    for (int i = 0; i < 3; ++i) { sa.std[i] = p->std[i]; sa.lo[i] = p->lo[i]; sa.hi[i] = p->hi[i]; }
    sa.total = (long long)h->cfg.K * h->cfg.N * 3; sa.N = h->cfg.N; sa.mu = mu; sa.sigma = sigma;
    return sa;
}

static int launch_cem_sample(rovmpc_handle *h, const PlanCtl &c, const PlanIter &it, const rovmpc_cem_params *p) {
    const double *mu = c.plan + it.in_off, *sigma = it.first ? nullptr : c.spread + it.in_off;      // sigma_0 = std
    if (h->prop_colored)
        return launch_proposal_sample(h, c, it, p->std, p->lo, p->hi, mu, sigma, c.single ? "CEM sampler" : "batched CEM sampler");
    const int gx = sampler_grid((long long)h->cfg.K * h->cfg.N * 3);
    if (c.single) {
        CemSampleArgs sa = cem_sample_args<CemSampleArgs>(h, it, p, mu, sigma);
        plan_single_in(sa, c, it);
        LAUNCH_SAMPLER(cem_sample_kernel, h, dim3(gx), sa, c.U);
        return launched(h, "CEM sampler");
    }
    CemSampleBatchArgs sa = cem_sample_args<CemSampleBatchArgs>(h, it, p, mu, sigma);
    sa.in = it.in;
    LAUNCH_SAMPLER(cem_sample_batch_kernel, h, dim3(gx, c.B), sa, c.U);
    return launched(h, "batched CEM sampler");
}

// one step of c's problems from host states, or a device loop of loop.T steps; then the mailbox rows into the caller's arrays
static int cem_run(rovmpc_handle *h, PlanCtl &c, const rovmpc_state *states, const PlanLoop &loop, const uint64_t *seeds, uint64_t step,
                   const rovmpc_cem_params *p, double *records_out = nullptr, double *means_out = nullptr, double *stds_out = nullptr,
                   int64_t *elites_out = nullptr, double *stats_out = nullptr) {
    int rc = plan_step(h, c, states, loop, seeds, step, p->n_iter,
                       [&](const PlanIter &it) { return launch_cem_sample(h, c, it, p); },
                       [&](const PlanIter &it) {
                           return launch_cem_update(h, c.J, c.U, p, c.plan + it.in_off, it.first ? nullptr : c.spread + it.in_off,
                                                    c.plan + it.out_off, c.spread + it.out_off, nullptr, nullptr, c.slab, c.tickets, it,
                                                    c.single ? nullptr : &c, h->stream);
                       });
    if (rc) return rc;
    const size_t C3 = 3 * (size_t)h->cfg.N, R = (size_t)rovmpc_result_len(h), E = (size_t)p->n_elite;
    for (size_t b = 0; records_out && b < (size_t)c.B; ++b) {
        const double *o = c.box.h_out + b * c.row;
        memcpy(records_out + b * R, o, R * sizeof(double));
        if (means_out) memcpy(means_out + b * C3, o + R, C3 * sizeof(double));
        if (stds_out) memcpy(stds_out + b * C3, o + R + C3, C3 * sizeof(double));
        if (stats_out) memcpy(stats_out + b * 4, o + R + 2 * C3, 4 * sizeof(double));
        if (elites_out) memcpy(elites_out + b * E, o + R + 2 * C3 + 4, E * sizeof(int64_t));
    }
    return take_device_errors(h);
}

extern "C" int rovmpc_cem_reset(rovmpc_handle *h, const double *mean) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!mean) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_cem_reset: null mean");
    return plan_reset(h, h->cem, 1, mean, cem_slab_bytes(h) / 8, cem_row_words(h), true);
}

extern "C" int rovmpc_cem_step(rovmpc_handle *h, const rovmpc_state *state, uint64_t seed, uint64_t step, const rovmpc_cem_params *p,
                               double *record_out, double *mean_out, double *std_out, int64_t *elite_out, double *stats_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!state || !record_out) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_cem_step: null pointer");
    int rc = cem_check_params(h, p);
    if (rc || (rc = plan_single_ready(h, h->cem, "step"))) return rc;
    return cem_run(h, h->cem, state, PlanLoop{}, &seed, step, p, record_out, mean_out, std_out, elite_out, stats_out);
}

extern "C" int rovmpc_cem_closed_loop_device(rovmpc_handle *h, const double *d_exo, int64_t T, int32_t feedback, uint64_t seed,
                                             uint64_t step0, const rovmpc_cem_params *p, double *d_rows) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = plan_loop_check(h, "rovmpc_cem_closed_loop_device", d_exo, T, feedback, d_rows);
    if (rc || (rc = cem_check_params(h, p)) || (rc = plan_single_ready(h, h->cem, "closed_loop_device"))) return rc;
    return cem_run(h, h->cem, nullptr, PlanLoop{d_exo, T, feedback, d_rows, cem_loop_row_words(h, p->n_elite)}, &seed, step0, p);
}

extern "C" int rovmpc_cem_last(rovmpc_handle *h, void *U_out, void *J_out) {
    return h ? plan_last(h, h->cem, U_out, J_out) : ROVMPC_ERR_INVALID;
}

extern "C" int rovmpc_cem_update_device(rovmpc_handle *h, const void *d_J, const void *d_U, const rovmpc_cem_params *p,
                                        const double *d_mean_in, const double *d_std_in, double *d_mean_out, double *d_std_out,
                                        int64_t *d_elite_out, double *d_stats, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!d_J || !d_U || !d_mean_in || !d_std_in || !d_mean_out || !d_std_out)
        FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_cem_update_device: null pointer");
    int rc = cem_check_params(h, p);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Slab &x = h->cem_slab_x;
    if ((rc = slab_alloc(h, x, cem_slab_bytes(h)))) return rc;
    return launch_cem_update(h, d_J, d_U, p, d_mean_in, d_std_in, d_mean_out, d_std_out, (long long *)d_elite_out, d_stats,
                             x.rows, x.ticket, PlanIter{}, nullptr, (hipStream_t)stream);
}

extern "C" int rovmpc_cem_reset_batch(rovmpc_handle *h, int32_t B, const double *means) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = check_batch_size(h, "rovmpc_cem_reset_batch", B);
    if (rc) return rc;
    if (!means) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_cem_reset_batch: null means");
    return plan_reset(h, h->cem_b, B, means, cem_slab_bytes(h) / 8, cem_row_words(h), true);
}

extern "C" int rovmpc_cem_step_batch(rovmpc_handle *h, int32_t B, const rovmpc_state *states, const uint64_t *seeds, uint64_t step,
                                     const rovmpc_cem_params *p, double *records_out, double *means_out, double *stds_out,
                                     int64_t *elites_out, double *stats_out) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = plan_batch_ready(h, h->cem_b, "rovmpc_cem_step_batch", B, !states || !seeds || !records_out, "states, seeds or records_out");
    if (rc || (rc = cem_check_params(h, p))) return rc;
    return cem_run(h, h->cem_b, states, PlanLoop{}, seeds, step, p, records_out, means_out, stds_out, elites_out, stats_out);
}

extern "C" int rovmpc_cem_closed_loop_batch_device(rovmpc_handle *h, int32_t B, const double *d_exo, int64_t T, int32_t feedback,
                                                   const uint64_t *seeds, uint64_t step0, const rovmpc_cem_params *p, double *d_rows) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = plan_batch_ready(h, h->cem_b, "rovmpc_cem_closed_loop_batch_device", B, !d_exo || !seeds || !d_rows, "d_exo, seeds or d_rows");
    if (rc || (rc = plan_loop_check(h, "rovmpc_cem_closed_loop_batch_device", d_exo, T, feedback, d_rows)) || (rc = cem_check_params(h, p))) return rc;
    return cem_run(h, h->cem_b, nullptr, PlanLoop{d_exo, T, feedback, d_rows, cem_loop_row_words(h, p->n_elite)}, seeds, step0, p);
}

extern "C" int rovmpc_cem_last_batch(rovmpc_handle *h, void *U_out, void *J_out) {
    return h ? plan_last(h, h->cem_b, U_out, J_out) : ROVMPC_ERR_INVALID;
}

// ---- timing ---------------------------------------------------------------------------------

extern "C" int rovmpc_timing_enable(rovmpc_handle *h, int32_t max_launches) {
    if (!h) return ROVMPC_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (auto &e : h->ev) (void)hipEventDestroy(e);
    h->ev.clear(); h->ev_used = 0; h->timing = max_launches > 0;
    for (int i = 0; i < 2 * max_launches; ++i) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    return ROVMPC_OK;
}

extern "C" int rovmpc_timing_read(rovmpc_handle *h, double *avg_ms, double *min_ms, int32_t *count) {
    if (!h) return ROVMPC_ERR_INVALID;
    double sum = 0, mn = 1e300;
    int n = 0;
    for (int i = 0; i + 1 < h->ev_used; i += 2) {
        HIPCHK(h, hipEventSynchronize(h->ev[i + 1]));
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        sum += ms; if (ms < mn) mn = ms; ++n;
    }
    if (avg_ms) *avg_ms = n ? sum / n : 0.0;
    if (min_ms) *min_ms = n ? mn : 0.0;
    if (count) *count = n;
    h->ev_used = 0;
    return ROVMPC_OK;
}

#ifdef ROVMPC_STAMPS
// Diagnostic library only: stamp slots per workgroup (the row length of what rovmpc_diag_read_stamps copies) ...
extern "C" int32_t rovmpc_diag_stamp_slots(void) { return RV_NSTAMP; }
// ... and copy the per-workgroup phase stamps of the last launch to the host.
extern "C" int rovmpc_diag_read_stamps(rovmpc_handle *h, unsigned long long *out, int32_t *nblocks) {
    if (!h || !out) return ROVMPC_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out, h->d_stamps, (size_t)h->nblocks * RV_NSTAMP * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemset(h->d_stamps, 0, (size_t)h->nblocks * RV_NSTAMP * sizeof(unsigned long long)));   // (slot 11 is OR-ed into)
    if (nblocks) *nblocks = h->nblocks;
    return ROVMPC_OK;
}
#endif

// ---- native collective ------------------------------------------------------------------------

struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;   // optional
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;
static std::mutex g_rccl_mu;

static const char *rccl_load() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return nullptr;
    // a bare SONAME first: binds to the copy already in the process (PyTorch bundles one)
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *lib = nullptr;
    for (const char *n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!lib) return "librccl.so not found (dlopen)";
    RcclApi a;
    a.lib = lib;
    a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))dlsym(lib, "ncclCommInitRank");
    a.AllReduce = (decltype(a.AllReduce))dlsym(lib, "ncclAllReduce");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(lib, "ncclCommDestroy");
    a.CommAbort = (decltype(a.CommAbort))dlsym(lib, "ncclCommAbort");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(lib, "ncclGetErrorString");
    a.Broadcast = (decltype(a.Broadcast))dlsym(lib, "ncclBroadcast");
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllReduce || !a.CommDestroy || !a.GetErrorString)
        return "librccl.so lacks an expected symbol";
    g_rccl = a;
    return nullptr;
}

#define NCCLCHK(h, call)                                                                               \
    do {                                                                                               \
        ncclResult_t _r = (call);                                                                      \
        if (_r != ncclSuccess) FAIL(h, ROVMPC_ERR_HIP, "%s failed: %s", #call, g_rccl.GetErrorString(_r)); \
    } while (0)

extern "C" int rovmpc_comm_unique_id(void *id128) {
    rovmpc_handle *nullh = nullptr;
    if (!id128) FAIL(nullh, ROVMPC_ERR_INVALID, "rovmpc_comm_unique_id: null argument");
    if (const char *why = rccl_load()) FAIL(nullh, ROVMPC_ERR_UNSUPPORTED, "%s", why);
    ncclUniqueId id;
    ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) FAIL(nullh, ROVMPC_ERR_HIP, "ncclGetUniqueId failed: %s", g_rccl.GetErrorString(r));
    memcpy(id128, &id, sizeof(id));
    return ROVMPC_OK;
}

static void comm_worker(rovmpc_handle *h) {
    (void)hipSetDevice(h->cfg.device);
    const size_t R = rovmpc_result_len(h);
    for (;;) {
        rovmpc_handle::CommJob job;
        {
            std::unique_lock<std::mutex> lk(h->comm_mu);
            h->comm_cv.wait(lk, [&] { return h->comm_stop || !h->comm_q.empty(); });
            if (h->comm_q.empty()) return;            // stop requested and nothing left to enqueue
            job = h->comm_q.front();
            h->comm_q.pop_front();
        }
        const int p = job.p;
        ncclComm_t comm = h->comms[job.c];
        hipStream_t cs = h->comm_streams[job.c];
        unsigned long long *f_rolled = h->d_flags + p, *f_consumed = h->d_flags + rovmpc_handle::NSLOT + p,
                           *f_bad = h->d_flags + 2 * rovmpc_handle::NSLOT + p;
        // twice the rollout's own limit: a rollout that gives up waiting for its slot row (after handoff_timeout_ms) still
        // publishes, marked bad, and the collective side must see THAT rather than race it to the same deadline
        const unsigned long long ticks = (unsigned long long)(2.0 * h->handoff_timeout_ms * 1e5);
        std::string err;
        // the rollout of this use publishes its row with a sequence number; no event on the caller's stream
        hipLaunchKernelGGL(wait_rolled_kernel, dim3(1), dim3(64), 0, cs, (const unsigned long long *)f_rolled, job.use, h->d_err, f_bad, ticks);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) err = std::string("wait kernel: ") + hipGetErrorString(e);
        if (err.empty()) {
            std::lock_guard<std::mutex> lk(h->comm_call_mu);
            if (h->comm_aborted || !h->comms[job.c]) {
                err = "the communicators were aborted (rovmpc_comm_abort)";
            } else {
                ncclResult_t r = g_rccl.AllReduce(h->d_slots[p], h->d_slots[p], (size_t)h->comm_world * R, ncclInt64, ncclMin, comm, cs);
                if (r != ncclSuccess) err = std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r);
            }
        }
        if (err.empty()) {
            hipLaunchKernelGGL(select_kernel, dim3(1), dim3(64), 0, cs, (const long long *)h->d_slots[p],
                               h->comm_world, (int)R, job.d_result, f_consumed, job.use, (const unsigned long long *)f_bad, job.inject,
                               job.ring, job.seq_theta, job.step_next);
            e = hipGetLastError();
            if (e != hipSuccess) err = std::string("select kernel: ") + hipGetErrorString(e);
        }
        // (no event per job: rovmpc_comm_join records one per collective stream when somebody needs the results)
        {
            std::lock_guard<std::mutex> lk(h->comm_mu);
            if (!err.empty() && h->comm_err.empty()) h->comm_err = err;
            ++h->comm_done[p];
        }
        h->comm_cv.notify_all();
    }
}

// Block the calling thread until the worker has ENQUEUED (not executed) every job on slot p.
int comm_wait_enqueued(rovmpc_handle *h, int p) {
    std::unique_lock<std::mutex> lk(h->comm_mu);
    h->comm_cv.wait(lk, [&] { return h->comm_done[p] == h->comm_submitted[p]; });
    if (!h->comm_err.empty()) FAIL(h, ROVMPC_ERR_HIP, "collective worker: %s", h->comm_err.c_str());
    return ROVMPC_OK;
}

extern "C" int rovmpc_comm_init(rovmpc_handle *h, const void *id128, int32_t rank, int32_t world) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!id128 || world < 1 || rank < 0 || rank >= world) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_comm_init: bad argument");
    if (h->comm) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_comm_init: communicator already initialised");
    if (const char *why = rccl_load()) FAIL(h, ROVMPC_ERR_UNSUPPORTED, "%s", why);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    NCCLCHK(h, g_rccl.CommInitRank(&h->comm, world, id, rank));
    h->comm_rank = rank; h->comm_world = world; h->comm_flip = 0; h->comm_rr = 0;
    h->comms[0] = h->comm; h->ncomm = 1;
    // The collective streams have the caller's (normal) priority.  Round 1 made them high-priority so that each got a
    // hardware queue of its own; measured in round 2 (world 1, all-reduce kept, `bench.py --force-collective`): with the
    // process's other high-priority stream that is four high-priority queues, and the rollout kernels on the caller's
    // normal-priority queue then last 55 us instead of 20 (57 us per step; one or two such streams: 22 us) -- a queue
    // of lower priority is starved while higher-priority queues hold unfinished dispatches (the waiting kernels).  At
    // equal priority nothing starves: 21.8 us per step with three communicators when the runtime may open eight hardware
    // queues (GPU_MAX_HW_QUEUES=8, which bench.py sets for its ranks), 25 us when they share the default four.  Sharing a
    // queue is safe: wait(i) is always submitted after rollout(i), select(i - NSLOT) before rollout(i).
    // ROVMPC_COMM_PRIO=hi brings the round-1 behaviour back.
    int lo = 0, hi = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    {
        const char *e = getenv("ROVMPC_COMM_PRIO");
        if (!(e && !strcmp(e, "hi"))) hi = 0;
    }
    HIPCHK(h, hipStreamCreateWithPriority(&h->comm_streams[0], hipStreamNonBlocking, hi));
    HIPCHK(h, hipMalloc((void **)&h->d_flags, 3 * rovmpc_handle::NSLOT * sizeof(unsigned long long)));
    HIPCHK(h, hipMemset(h->d_flags, 0, 3 * rovmpc_handle::NSLOT * sizeof(unsigned long long)));
    {
        // More communicators (ROVMPC_COMMS=1 keeps the single one).  Rank 0 draws their ids and hands them round
        // with ncclBroadcast on the first communicator; every rank then agrees (one all-reduce(min) of a flag) that
        // all of them came up -- otherwise everybody drops back to the single communicator.
        int want = rovmpc_handle::NCOMM_MAX;
        if (const char *e = getenv("ROVMPC_COMMS")) want = atoi(e);
        if (want > rovmpc_handle::NCOMM_MAX) want = rovmpc_handle::NCOMM_MAX;
        if (want > 1 && g_rccl.Broadcast) {
            const int extra = want - 1;
            ncclUniqueId ids[rovmpc_handle::NCOMM_MAX];
            memset(ids, 0, sizeof(ids));
            int ok = 1;
            if (rank == 0)
                for (int c = 0; c < extra; ++c)
                    if (g_rccl.GetUniqueId(&ids[c]) != ncclSuccess) ok = 0;
            void *d_ids = nullptr; int *d_ok = nullptr;
            HIPCHK(h, hipMalloc(&d_ids, sizeof(ids)));
            HIPCHK(h, hipMalloc((void **)&d_ok, sizeof(int)));
            HIPCHK(h, hipMemcpy(d_ids, ids, sizeof(ids), hipMemcpyHostToDevice));
            NCCLCHK(h, g_rccl.Broadcast(d_ids, d_ids, sizeof(ids), ncclChar, 0, h->comm, h->comm_streams[0]));
            HIPCHK(h, hipStreamSynchronize(h->comm_streams[0]));
            HIPCHK(h, hipMemcpy(ids, d_ids, sizeof(ids), hipMemcpyDeviceToHost));
            int made = 0;
            for (int c = 0; c < extra && ok; ++c) {
                if (g_rccl.CommInitRank(&h->comms[1 + c], world, ids[c], rank) != ncclSuccess) { ok = 0; break; }
                ++made;
                if (hipStreamCreateWithPriority(&h->comm_streams[1 + c], hipStreamNonBlocking, hi) != hipSuccess) { ok = 0; break; }
            }
            HIPCHK(h, hipMemcpy(d_ok, &ok, sizeof(int), hipMemcpyHostToDevice));
            NCCLCHK(h, g_rccl.AllReduce(d_ok, d_ok, 1, ncclInt32, ncclMin, h->comm, h->comm_streams[0]));
            HIPCHK(h, hipStreamSynchronize(h->comm_streams[0]));
            HIPCHK(h, hipMemcpy(&ok, d_ok, sizeof(int), hipMemcpyDeviceToHost));
            (void)hipFree(d_ids); (void)hipFree(d_ok);
            if (ok) {
                h->ncomm = want;
            } else {
                for (int c = 1; c <= made; ++c) { (void)g_rccl.CommDestroy(h->comms[c]); h->comms[c] = nullptr; }
                for (int c = 1; c < rovmpc_handle::NCOMM_MAX; ++c)
                    if (h->comm_streams[c]) { (void)hipStreamDestroy(h->comm_streams[c]); h->comm_streams[c] = nullptr; }
            }
        }
    }
    const size_t R = rovmpc_result_len(h);
    for (int i = 0; i < rovmpc_handle::NSLOT; ++i) {
        HIPCHK(h, hipMalloc((void **)&h->d_slots[i], (size_t)world * R * sizeof(long long)));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_selected[i], hipEventDisableTiming));
        h->slot_used[i] = false;
        h->slot_uses[i] = 0;
        h->comm_submitted[i] = h->comm_done[i] = 0;
    }
    h->comm_stop = false;
    h->comm_err.clear();
    h->comm_thread = std::thread(comm_worker, h);
    return ROVMPC_OK;
}

// Where the side streams live.  A hardware queue whose head packet waits (the wait kernel, an RCCL kernel waiting for its
// peers, a closed-loop step waiting for its predecessor's hand-off) delays the completion of every kernel on the other
// queue of its command-processor pipe by tens of microseconds -- measured: rollouts of 55 us instead of 20 when the
// caller's queue and a collective queue are such a pair, which depends on nothing but the order in which the process
// happened to create its streams (queue ids k and k + 4 share a pipe; tools/ubench/queue_collision.hip).  So side streams
// are CHOSEN: when the caller's stream is known, candidates of normal and of high priority (the `seed` streams first) are
// probed against it -- a parked lane on one, a few short grids on the other, both ways; a colliding or queue-sharing
// candidate shows up as a multiple of the undisturbed time -- and against the ones already chosen, until `want` are found.
// Candidates created here and not chosen are destroyed.  Every wait is bounded (2 ms); the probe takes a few milliseconds.
// Returns the chosen streams (possibly fewer than `want`, possibly none) and a one-line report.
int choose_side_streams(rovmpc_handle *h, hipStream_t caller, const std::vector<hipStream_t> &seed, int want,
                        std::vector<hipStream_t> &chosen, std::string &log) {
    unsigned long long *d_flag = nullptr; double *d_x = nullptr;
    HIPCHK(h, hipMalloc((void **)&d_flag, 8));
    HIPCHK(h, hipMemset(d_flag, 0, 8));
    HIPCHK(h, hipMalloc((void **)&d_x, 256 * 64 * sizeof(double)));
    HIPCHK(h, hipMemset(d_x, 0, 256 * 64 * sizeof(double)));
    unsigned long long seq = 0;
    const int M = 6;
    // time of M short grids + the releasing kernel on `on` while a lane is parked on `parked`
    auto probe = [&](hipStream_t on, hipStream_t parked, bool have_parked) -> double {
        double best = 1e30;
        for (int rep = 0; rep < 3; ++rep) {
            ++seq;
            const auto t0 = std::chrono::steady_clock::now();
            if (have_parked) hipLaunchKernelGGL(probe_park_kernel, dim3(1), dim3(64), 0, parked, (const unsigned long long *)d_flag, seq, 200000ULL);
            for (int m = 0; m < M; ++m) hipLaunchKernelGGL(probe_short_kernel, dim3(256), dim3(64), 0, on, d_x);
            hipLaunchKernelGGL(probe_raise_kernel, dim3(1), dim3(64), 0, on, d_flag, seq);
            (void)hipStreamSynchronize(on);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (have_parked) (void)hipStreamSynchronize(parked);
            if (us < best) best = us;
        }
        return best;
    };
    (void)probe(caller, nullptr, false);                       // warm: code objects loaded, queues bound
    const double base = probe(caller, nullptr, false);
    const double limit = 1.5 * base + 15.0;                    // a colliding pair costs >= 20 us per kernel, M + 1 kernels
    int lo = 0, hi = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    std::vector<hipStream_t> cand(seed);
    for (int j = 0; j < 12; ++j) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, j < 6 ? 0 : hi) != hipSuccess) continue;
        hipLaunchKernelGGL(probe_short_kernel, dim3(1), dim3(64), 0, st, d_x);      // bind it to its queue
        (void)hipStreamSynchronize(st);
        cand.push_back(st);
    }
    std::vector<size_t> pick;
    char line[160];
    snprintf(line, sizeof(line), "undisturbed %.0f us, limit %.0f us;", base, limit);
    log = line;
    for (size_t j = 0; j < cand.size() && (int)pick.size() < want; ++j) {
        double worst = probe(caller, cand[j], true);                               // the candidate parks, the caller's stream works
        if (worst <= limit) {
            const double back = probe(cand[j], caller, true);                      // and the other way round
            if (back > worst) worst = back;
        }
        for (size_t q = 0; q < pick.size() && worst <= limit; ++q) {
            double t = probe(cand[pick[q]], cand[j], true);
            if (t > worst) worst = t;
            if (worst <= limit) { t = probe(cand[j], cand[pick[q]], true); if (t > worst) worst = t; }
        }
        snprintf(line, sizeof(line), " %zu:%s%.0f%s", j, j < seed.size() ? "seed " : (j < seed.size() + 6 ? "" : "hi "), worst, worst <= limit ? "*" : "");
        log += line;
        if (worst <= limit) pick.push_back(j);
    }
    std::vector<bool> used(cand.size(), false);
    chosen.clear();
    for (size_t q : pick) { chosen.push_back(cand[q]); used[q] = true; }
    for (size_t j = seed.size(); j < cand.size(); ++j)
        if (!used[j]) (void)hipStreamDestroy(cand[j]);
    (void)hipFree(d_flag); (void)hipFree(d_x);
    return ROVMPC_OK;
}

// The collective streams: one per communicator where the probe finds that many, else the communicators share what it found;
// nothing found (or ROVMPC_COMM_PLACE=0): the streams of rovmpc_comm_init stay.
int place_comm_streams(rovmpc_handle *h, hipStream_t caller) {
    h->comm_placed = true;
    if (const char *e = getenv("ROVMPC_COMM_PLACE")) if (!strcmp(e, "0")) { h->comm_placement = "off (ROVMPC_COMM_PLACE=0)"; return ROVMPC_OK; }
    std::vector<hipStream_t> seed, chosen;
    for (int c = 0; c < h->ncomm; ++c)
        if (h->comm_streams[c]) seed.push_back(h->comm_streams[c]);
    std::string log;
    int rc = choose_side_streams(h, caller, seed, h->ncomm, chosen, log);
    if (rc) return rc;
    char line[96];
    if (!chosen.empty()) {
        for (hipStream_t st : seed) {
            bool kept = false;
            for (hipStream_t c : chosen) kept = kept || c == st;
            if (!kept) (void)hipStreamDestroy(st);
        }
        for (int c = 0; c < h->ncomm; ++c) h->comm_streams[c] = chosen[(size_t)c % chosen.size()];
        snprintf(line, sizeof(line), " -> %zu stream(s) for %d communicator(s)", chosen.size(), h->ncomm);
    } else {
        snprintf(line, sizeof(line), " -> no candidate passed, streams of rovmpc_comm_init kept");
    }
    h->comm_placement = log + line;
    if (getenv("ROVMPC_COMM_PLACE_VERBOSE")) fprintf(stderr, "[rovmpc] collective stream placement: %s\n", h->comm_placement.c_str());
    return ROVMPC_OK;
}

// Takes the next collective slot p for one sharded step and writes the step's sharding and slot hand-off options into o.
// Slot buffer p is free once the select of NSLOT steps ago has read it.  On the host: that job has been handed
// to the collective stream (bounds the queue).  On the GPU: the rollout's last workgroup waits for
// consumed[p] >= uses - 1 before it writes the row and then publishes rolled[p] = uses; the collective stream
// polls that (wait_rolled_kernel).  The caller's stream carries rollout kernels only.
int comm_take_slot(rovmpc_handle *h, StepOpts &o, int &p) {
    p = h->comm_flip;
    h->comm_flip = (h->comm_flip + 1) % rovmpc_handle::NSLOT;
    if (h->slot_used[p]) {
        int rc = comm_wait_enqueued(h, p);
        if (rc) return rc;
    }
    h->slot_used[p] = true;
    const unsigned long long use = ++h->slot_uses[p];
    o.slots = h->d_slots[p]; o.rank = h->comm_rank; o.world = h->comm_world;
    o.flag_consumed = h->d_flags + rovmpc_handle::NSLOT + p; o.consumed_need = use - 1;
    o.flag_rolled = h->d_flags + p; o.rolled_seq = use;
    o.slot_bad = h->d_flags + 2 * rovmpc_handle::NSLOT + p;
    o.inject = 0;
    if (h->inject_skip_rolled > 0) { --h->inject_skip_rolled; o.inject |= 1; }
    if (h->inject_skip_consumed > 0) { --h->inject_skip_consumed; o.inject |= 2; }
    return ROVMPC_OK;
}

// Hands the collective and select of the step launched with o on slot p to the worker thread; the global record goes to
// d_result.  Closed loop: the select also hands theta over to step `step_next` through ring / seq_theta.
void comm_submit(rovmpc_handle *h, int p, const StepOpts &o, double *d_result, double *ring, unsigned long long *seq_theta, long long step_next) {
    {
        std::lock_guard<std::mutex> lk(h->comm_mu);
        h->comm_q.push_back({p, d_result, o.rolled_seq, (int)(h->comm_rr++ % (unsigned long long)h->ncomm), o.inject, ring, seq_theta, step_next});
        ++h->comm_submitted[p];
    }
    h->comm_cv.notify_all();
}

extern "C" int rovmpc_step_device_allreduce(rovmpc_handle *h, const double *d_state, const void *d_U, int64_t k_offset,
                                            double *d_result, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!h->comm) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_step_device_allreduce: call rovmpc_comm_init first");
    if (!d_state || !d_U || !d_result) FAIL(h, ROVMPC_ERR_INVALID, "rovmpc_step_device_allreduce: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!h->comm_placed) {
        int rc = place_comm_streams(h, s);
        if (rc) return rc;
    }
    StepOpts o;
    o.k_offset = k_offset;
    int p, rc = comm_take_slot(h, o, p);
    if (rc) return rc;
    if ((rc = enqueue_step(h, d_state, d_U, h->d_result, s, o))) return rc;
    comm_submit(h, p, o, d_result);
    return ROVMPC_OK;
}

extern "C" int rovmpc_comm_join(rovmpc_handle *h, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!h->comm) return ROVMPC_OK;
    bool any = false;
    for (int i = 0; i < rovmpc_handle::NSLOT; ++i) {
        if (!h->slot_used[i]) continue;
        int rc = comm_wait_enqueued(h, i);          // the worker has handed every job of this slot to its stream
        if (rc) return rc;
        any = true;
    }
    if (!any) return ROVMPC_OK;
    // the worker is idle now, so the collective streams may be touched from this thread: one event per stream
    for (int c = 0; c < h->ncomm; ++c) {
        HIPCHK(h, hipEventRecord(h->ev_selected[c], h->comm_streams[c]));
        HIPCHK(h, hipStreamWaitEvent((hipStream_t)stream, h->ev_selected[c], 0));
    }
    // a hand-off that gave up in a step the GPU has already executed is reported here (the join itself does not block)
    return take_device_errors(h);
}

extern "C" int rovmpc_comm_sync(rovmpc_handle *h, void *stream) {
    if (!h) return ROVMPC_ERR_INVALID;
    int rc = rovmpc_comm_join(h, stream);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    return take_device_errors(h);
}

// Callable from ANOTHER thread while steps are in flight (that is its purpose): a collective that never completes -- a peer
// that died, an ordering fault -- leaves its kernel waiting on the collective stream for ever and rovmpc_comm_sync with
// it.  ncclCommAbort makes those kernels leave; the GPU-side hand-off waits behind them give up on their own clocks
// (handoff_timeout_ms), the steps' records carry NaN costs and rovmpc_comm_sync returns its error.  Afterwards the handle
// issues no collective any more: rovmpc_comm_destroy, then rovmpc_comm_init again or another path.
extern "C" int rovmpc_comm_abort(rovmpc_handle *h) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!h->comm) return ROVMPC_OK;
    if (!g_rccl.CommAbort) FAIL(h, ROVMPC_ERR_UNSUPPORTED, "librccl has no ncclCommAbort");
    ncclComm_t doomed[rovmpc_handle::NCOMM_MAX] = {};
    {
        std::lock_guard<std::mutex> lk(h->comm_call_mu);       // the worker is not inside ncclAllReduce while this is held
        h->comm_aborted = true;
        for (int c = 0; c < rovmpc_handle::NCOMM_MAX; ++c) { doomed[c] = h->comms[c]; h->comms[c] = nullptr; }
    }
    for (int c = 0; c < rovmpc_handle::NCOMM_MAX; ++c)
        if (doomed[c]) (void)g_rccl.CommAbort(doomed[c]);      // frees the communicator: no ncclCommDestroy afterwards
    return ROVMPC_OK;
}

extern "C" const char *rovmpc_comm_placement(const rovmpc_handle *h) { return h ? h->comm_placement.c_str() : ""; }

extern "C" int rovmpc_comm_destroy(rovmpc_handle *h) {
    if (!h) return ROVMPC_ERR_INVALID;
    if (!h->comm) return ROVMPC_OK;
    (void)hipSetDevice(h->cfg.device);
    {
        std::lock_guard<std::mutex> lk(h->comm_mu);
        h->comm_stop = true;
    }
    h->comm_cv.notify_all();
    if (h->comm_thread.joinable()) h->comm_thread.join();
    for (int c = 0; c < rovmpc_handle::NCOMM_MAX; ++c)
        if (h->comm_streams[c]) (void)hipStreamSynchronize(h->comm_streams[c]);
    for (int c = 0; c < rovmpc_handle::NCOMM_MAX; ++c)
        if (h->comms[c]) { (void)g_rccl.CommDestroy(h->comms[c]); h->comms[c] = nullptr; }
    h->comm = nullptr; h->ncomm = 0;
    if (h->d_flags) { (void)hipFree(h->d_flags); h->d_flags = nullptr; }
    for (int i = 0; i < rovmpc_handle::NSLOT; ++i) {
        if (h->d_slots[i]) (void)hipFree(h->d_slots[i]);
        if (h->ev_selected[i]) (void)hipEventDestroy(h->ev_selected[i]);
        h->d_slots[i] = nullptr; h->ev_selected[i] = nullptr;
    }
    for (int c = 0; c < rovmpc_handle::NCOMM_MAX; ++c) {
        if (!h->comm_streams[c]) continue;
        hipStream_t st = h->comm_streams[c];
        for (int d = c; d < rovmpc_handle::NCOMM_MAX; ++d)          // communicators may share a stream after the placement
            if (h->comm_streams[d] == st) h->comm_streams[d] = nullptr;
        (void)hipStreamDestroy(st);
    }
    h->comm_placed = false;
    h->comm_aborted = false;
    return take_device_errors(h);       // anything raised since the last rovmpc_comm_sync
}
