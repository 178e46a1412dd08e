// rovmpc_internal.h -- what the host units of librovmpc.so (rovmpc.hip, helpers_host.hip, closed_loop_host.hip) share: the handle and its parts,
// the error macros, the options of one rollout launch (StepOpts), what a launch runs (Launchable) and the host functions that
// more than one unit calls.  Nothing declared here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include <rccl/rccl.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "rollout_kernels.h"

#pragma GCC visibility push(hidden)

using namespace rovmpc;

extern thread_local std::string g_create_error;      // last error of a call without a handle (rovmpc.hip)

// Where the kernel that ends a step leaves its results for the host: a block of doubles in mapped host memory and, behind
// it, the sequence word that kernel releases at system scope and the host spins on (mailbox_wait).
struct Mailbox {
    double *h_out = nullptr, *d_out = nullptr;
    unsigned long long *h_done = nullptr, *d_done = nullptr;
    unsigned long long seq = 0;                  // last sequence number handed out
};

// Partial results of an update kernel's workgroups and the ticket word its last workgroup re-arms (zeroed once): the set of
// rovmpc_*_update_device; a controller keeps one per problem in its PlanCtl.
struct Slab { void *rows = nullptr; unsigned *ticket = nullptr; };

// What a controller that iterates on a plan (MPPI: the nominal; CEM: mean and spread) owns, for B problems side by side (every
// per-problem array the one-problem array repeated B times): candidate tensors, costs, states and records of its own (the
// other entry points' buffers are never touched), the plans double-buffered by iteration, the update's slabs and tickets
// and the mailbox [B][row] of its step.  Made at rovmpc_*_reset_batch, again when B changes.  `single`: the one-problem
// controller of rovmpc_*_reset / _step, made at its first reset with B = 1; state and seed reach its sampler as kernel
// arguments, so it has no staging block and no seeds.
struct PlanCtl {
    const char *name, *abi;                      // "MPPI", "mppi": for the messages
    bool single;
    int B = 0;                                   // 0: no reset yet
    void *U = nullptr, *J = nullptr;             // T [B][K][N][3], T [B][K]
    double *state = nullptr, *record = nullptr;  // [B][16], [B][result_len]
    unsigned long long *seeds = nullptr;         // [B]: kept by the first sampler of a step for the later ones (batched)
    double *plan = nullptr, *spread = nullptr;   // [2][B][3N] each; spread: CEM only
    int cur = 0;                                 // half of plan (and spread) holding the handle's
    void *slab = nullptr;                        // [B] slabs of slab_stride 64-bit words
    unsigned *tickets = nullptr;                 // [B] of the problems' updates, then the step's
    size_t slab_stride = 0, row = 0;             // row: 64-bit words per problem of the mailbox
    double *h_stage = nullptr, *d_stage = nullptr;   // mapped: states [B][16], seeds [B] of the step being enqueued (batched)
    Mailbox box;                                 // [B][row]
    unsigned long long steps = 0;
};

struct rovmpc_handle {
    rovmpc_config cfg;
    hipStream_t stream = nullptr;
    std::string err;
    // model
    bool has_model = false, builtin = false;
    int model_kind = MODEL_INTERP;   // MODEL_BUILTIN | MODEL_INTERP | MODEL_JIT
    hipFunction_t jit_fn = nullptr;  // MODEL_JIT: kernel of the run-time specialised module
    int jit_ckc = 0;                 // candidates per workgroup the module was specialised for (0: run-time)
    hipFunction_t jit_fn_step = nullptr;   //            its pipelined closed-loop step entry
    int jit_gi = 0, jit_ts = 0;            //            structure found in the rows (ROVMPC_JIT_GI / ROVMPC_JIT_TS of rollout_kernels.h)
    hipStream_t pipe_streams[2] = {nullptr, nullptr};     // pipelined closed loop: launches alternate between the two
    bool pipe_placed = false, pipe_stream_owned = false;  // [1] probed against the caller's stream; replaced by one of the handle's own
    std::string pipe_placement;
    hipEvent_t pipe_ev[3] = {nullptr, nullptr, nullptr};
    // closed loop with GPU-side hand-off (pipelined form): sequence words [2] + state ring [4][4] in one block,
    // and the granule / trajectory hand-off buffers by step parity
    unsigned long long *d_step_seq = nullptr;
    unsigned long long *d_cl_granules = nullptr;
    double *d_cl_blk_traj = nullptr;
    int cl_form = 0;                 // form of the last closed-loop call (rovmpc_closed_loop_form)
    int n_feat = 0;
    double mean[ROVMPC_MAX_FEATURES], scale[ROVMPC_MAX_FEATURES];
    int n_th = 0, n_ga = 0, n_consts = 0;
    unsigned used_planes = 0xffffffffu;   // exogenous planes read by the loaded expressions
    int32_t *d_code_th = nullptr, *d_code_ga = nullptr;
    void *d_consts = nullptr;        // T
    double *d_consts64 = nullptr;    // double (utility kernels)
    void *d_Rtab = nullptr;          // T [N][9]
    void *d_k = nullptr;             // RolloutConsts<T>
    bool has_rtab = false;
    // launch geometry / workspace
    int CK = 0, nblocks = 0, NT = 0;
    int n_cu = 256;                  // compute units of the device (multiProcessorCount)
    size_t lds_bytes = 0, esz = 8;
    void *d_U = nullptr, *d_J = nullptr, *d_traj_all = nullptr;
    double *d_state = nullptr, *d_blk_traj = nullptr, *d_result = nullptr;
    unsigned long long *d_granules = nullptr;  // [gran_stride(max_blocks, N)] tagged hand-off granules: costs, then best trajectories
    unsigned *epoch_ctr = nullptr;            // launches issued (host counter; tag of the next launch = ++*epoch_ctr, never 0)
    unsigned long long *d_stamps = nullptr;   // diagnostic library only
    void *d_gtab = nullptr;                   // shared gamma table of a launch (long horizons) + its epoch tag behind it
    // error word: pinned host memory mapped into the device (ERR_* bits of rollout_kernels.h), raised at system scope by
    // the kernels' give-up paths, read and cleared by rovmpc_comm_sync / rovmpc_device_status
    unsigned *h_err = nullptr, *d_err = nullptr;
    double handoff_timeout_ms = 10000.0;      // give-up time of the GPU-side hand-off waits (rovmpc_set_option)
    int inject_skip_rolled = 0, inject_skip_consumed = 0;   // test hooks: the next N steps lose that publication
    int track_chunk = 256;                    // frames per launch of rovmpc_track_markers* (rovmpc_set_option)
    void *d_score_prog = nullptr;             // rovmpc_score_rows_device: the programs and lengths of the last call,
    size_t score_prog_bytes = 0;              // their host copy (the source of the upload) and the event behind that upload
    std::vector<unsigned char> score_prog_host;
    hipEvent_t score_prog_ev = nullptr;
    double *d_discover_partial = nullptr;     // rovmpc_discover_rows*: the chunk partials of the last call, grown on demand
    size_t discover_partial_n = 0;
    struct CalibWork *calib = nullptr;        // rovmpc_calibrate_cable*: its working buffers, grown on demand (helpers_host.hip)
    // rovmpc_mpc_step_sampled: two candidate tensors (the sampler of step s+1 reads the winner of step s for the warm
    // start) and the mailbox of the record (its sequence numbers are samp_steps)
    void *d_Us[2] = {nullptr, nullptr};
    Mailbox samp_box;
    unsigned long long samp_steps = 0;
    double *d_best = nullptr;                    // [2][N][3]: winner's sequence of the last fused-sampling steps, by step parity
    unsigned long long *d_blk_u = nullptr;       // [max_blocks][6 N] tagged granules + [max_blocks][3 N] doubles: per-workgroup best controls of a fused-sampling step
    // what the last sampled step drew with (rovmpc_sampled_candidates re-draws the tensor for inspection)
    unsigned long long last_seed = 0, last_step = 0; double last_mean[3] = {}, last_std[3] = {}; int last_warm = 0; bool last_fused = false;
    // MPPI (rovmpc_mppi_*): mailbox [record, nu*, stats]; CEM (rovmpc_cem_*): [record, mu*, sigma*, stats, elite list]
    PlanCtl mppi{"MPPI", "mppi", true}, cem{"CEM", "cem", true};
    PlanCtl mppi_b{"MPPI", "mppi", false}, cem_b{"CEM", "cem", false};
    Slab mppi_slab_x, cem_slab_x;                // of rovmpc_*_update_device (allocated at its first call)
    // shaping of the controllers' proposal (rovmpc_set_noise_correlation, rovmpc_mppi_set_bounds); the defaults launch the
    // white samplers and the unbounded update
    double prop_beta[3] = {0.0, 0.0, 0.0}, prop_root[3] = {1.0, 1.0, 1.0};    // root = sqrt((1 - beta)(1 + beta))
    double mppi_lo[3] = {-INFINITY, -INFINITY, -INFINITY}, mppi_hi[3] = {INFINITY, INFINITY, INFINITY};
    bool prop_colored = false, mppi_boxed = false;
    // navigation cost of the controllers (rovmpc_set_nav_cost): the setting, its tracks [nav_Bt][nav_Tr][3] and spheres
    // [ROVMPC_NAV_MAX_SPHERES][4] in device memory; unset: nav_cost_kernel is not launched
    bool nav_on = false;
    rovmpc_nav_cost nav = {};
    double *d_nav_track = nullptr, *d_nav_spheres = nullptr;
    size_t nav_track_cap = 0;                    // doubles allocated behind d_nav_track
    int nav_Bt = 0; long long nav_Tr = 0;
    // tether keep-out cost of the controllers (rovmpc_set_tether_cost): the setting, its spheres in device memory and the
    // buffer [tether_cap][K][N+1][2] the rollout stores its trajectories in; unset: tether_cost_kernel is not launched and
    // the rollout gets no trajectory buffer
    bool tether_on = false;
    rovmpc_tether_cost tether = {};
    double *d_tether_spheres = nullptr;
    void *d_tether_traj = nullptr;
    int tether_cap = 0;                          // problems d_tether_traj holds
    // batched launches: workspace for `batch_cap` problems
    int batch_cap = 0, last_batch = 1;           // last_batch: B of the last launch that wrote the handle's own cost buffers
    void *d_Jb = nullptr; double *d_blk_trajb = nullptr; unsigned long long *d_granulesb = nullptr;
    double *h_result = nullptr;      // pinned
    // native collective (rovmpc_comm_*)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0, comm_flip = 0;
    static constexpr int NSLOT = 4;       // collectives in flight (RCCL's small all-reduce is ~2 rollouts long)
    // Several communicators (each with a high-priority stream of its own), used round-robin by the slots:
    // collectives on one communicator serialise, and a latency-bound 3 KB all-reduce over 8 GPUs lasts longer than a
    // rollout -- with more than one communicator the collectives of consecutive steps overlap each other as well as
    // the rollouts.  Three by default: with the caller's stream that is four hardware queues, the runtime's default
    // limit (a fifth stream was measured to cost 80 us per step).  comms[0] == comm.
    static constexpr int NCOMM_MAX = 3;
    ncclComm_t comms[NCOMM_MAX] = {};
    hipStream_t comm_streams[NCOMM_MAX] = {};
    int ncomm = 0;
    bool comm_placed = false;             // place_comm_streams has run (first rovmpc_step_device_allreduce)
    bool comm_aborted = false;            // rovmpc_comm_abort: no further collective is issued (guarded by comm_call_mu)
    std::mutex comm_call_mu;              // the worker's [aborted? -> ncclAllReduce] against rovmpc_comm_abort
    std::string comm_placement;           // what it found (rovmpc_get_info "comm_placement")
    // GPU-side hand-off between the caller's stream and the collective streams (no events on the caller's stream:
    // an event record costs ~3 us and a cross-stream wait ~6 us of its timeline per step, measured):
    // rolled[p] = uses of slot p whose rollout has published its row; consumed[p] = uses whose select has read it.
    unsigned long long *d_flags = nullptr;             // [3][NSLOT]: rolled, consumed, bad use
    unsigned long long slot_uses[NSLOT] = {};
    long long *d_slots[NSLOT] = {};
    hipEvent_t ev_selected[NSLOT] = {};   // recorded at rovmpc_comm_join, one per collective stream
    bool slot_used[NSLOT] = {};
    // the collective is enqueued by a worker thread so its host cost (ncclAllReduce is ~20 us of
    // host time per call) overlaps the enqueue of the next rollout
    struct CommJob { int p; double *d_result; unsigned long long use; int c; int inject;
                     double *ring; unsigned long long *seq_theta; long long step_next; };     // (closed loop: the select hands theta over)
    unsigned long long comm_rr = 0;       // steps issued: communicator of a step = comm_rr % ncomm (same on every rank)
    std::thread comm_thread;
    std::mutex comm_mu;
    std::condition_variable comm_cv;
    std::deque<CommJob> comm_q;
    unsigned long long comm_submitted[NSLOT] = {}, comm_done[NSLOT] = {};
    bool comm_stop = false;
    std::string comm_err;
    // timing
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    bool timing = false;
};

#define FAIL(h, code, ...)                                        \
    do {                                                          \
        char _b[512];                                             \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                    \
        if (h) (h)->err = _b; else g_create_error = _b;           \
        return (code);                                            \
    } while (0)

#define HIPCHK(h, call)                                                                     \
    do {                                                                                    \
        hipError_t _e = (call);                                                             \
        if (_e != hipSuccess)                                                               \
            FAIL(h, ROVMPC_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),  \
                 __FILE__, __LINE__);                                                       \
    } while (0)

// Geometry of one launch: B problems of K candidates each in the grid (B = 1: the handle's own geometry).
struct Geo { int CK, NT, nblocks; };

// What one rollout launch is asked for beyond state, candidates and record, in the groups of RolloutArgs.  The default is the
// plain single step; a launch reads its options from this value alone, never from the handle.
struct StepOpts {
    void *J = nullptr, *traj_all = nullptr;      // costs (null: the handle's d_J, d_Jb of a batch), every candidate's trajectory
    long long k_offset = 0;                      // sharding: first global candidate, slot row image, rank / world
    long long *slots = nullptr;
    int rank = 0, world = 1;
    double *result_host = nullptr;               // mailbox the step publishes its record into, with done_seq behind it
    unsigned long long *done_flag = nullptr, done_seq = 0;
    const unsigned long long *flag_consumed = nullptr;      // slot hand-off of the native collective (comm_take_slot)
    unsigned long long consumed_need = 0;
    unsigned long long *flag_rolled = nullptr, rolled_seq = 0, *slot_bad = nullptr;
    int inject = 0;
    const double *plant_next = nullptr;          // closed loop: plant update fused into the step's epilogue
    double *plant_state = nullptr;
    int plant_feedback = 0;
    int B = 1;                                   // problems in the grid
    // the plain single-problem step takes the lean instantiation of the compiled-in kernel (see rollout_body)
    bool lean() const { return B == 1 && !slots && !flag_consumed && !flag_rolled && !result_host && !done_flag && !plant_next; }
};

// Which kernel a launch runs and what it is launched with.
enum LaunchKind { LAUNCH_PLAIN, LAUNCH_SAMPLED, LAUNCH_STEP };     // rollout_kernel*, rollout_kernel_sampled, closed_loop_step_kernel*
struct Launchable {
    const void *fn = nullptr;        // instance compiled into the library (compiled-in model or interpreter), or
    hipFunction_t mod = nullptr;     // function of the hiprtc module
    size_t lds = 0;                  // dynamic LDS, bytes
};

// ---- helpers_host.hip ----
void calib_free(rovmpc_handle *h);           // the working buffers of rovmpc_calibrate_cable*, for rovmpc_destroy

// ---- rovmpc.hip ----
Geo launch_geometry(const rovmpc_handle *h, int B);
const char *validate_code(const int32_t *code, int n, int n_feat, int n_consts);
hipError_t rollout_launchable(const rovmpc_handle *h, LaunchKind kind, const Geo &g, const StepOpts &o, Launchable &k);
hipError_t launchable_capacity(const rovmpc_handle *h, const Launchable &k, int NT, int *capacity);
template <typename T> void fill_args(const rovmpc_handle *h, RolloutArgs<T> &a, const double *d_state, const void *d_U,
                                     double *d_result, const Geo &g, const StepOpts &o);      // T = double, float
template <typename T> hipError_t launch_rollout(const rovmpc_handle *h, const Launchable &k, RolloutArgs<T> &a, int B, hipStream_t s,
                                                const HandoffArgs *p = nullptr);
int check_ready(rovmpc_handle *h);
int enqueue_step(rovmpc_handle *h, const double *d_state, const void *d_U, double *d_result, hipStream_t s, const StepOpts &o = StepOpts());
int launched(rovmpc_handle *h, const char *what);
int comm_wait_enqueued(rovmpc_handle *h, int p);
int comm_take_slot(rovmpc_handle *h, StepOpts &o, int &p);
void comm_submit(rovmpc_handle *h, int p, const StepOpts &o, double *d_result, double *ring = nullptr, unsigned long long *seq_theta = nullptr,
                 long long step_next = 0);
int choose_side_streams(rovmpc_handle *h, hipStream_t caller, const std::vector<hipStream_t> &seed, int want,
                        std::vector<hipStream_t> &chosen, std::string &log);
int place_comm_streams(rovmpc_handle *h, hipStream_t caller);

#pragma GCC visibility pop
