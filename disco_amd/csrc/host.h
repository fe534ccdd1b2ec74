// Host-side internals of libdisco_hip.so shared by its translation units (api_*.hip): the context, the error / device-guard /
// stage-timer helpers, and the stage functions the whole-path entry points chain.  Not part of the C ABI (include/disco_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/disco_hip.h"
#include "common.h"
#include "dispatch.h"


using disco::c32;

// per-context options (disco_set_option / disco_get_option); the environment variable of the same meaning presets the value at
// disco_create and is never looked at again
enum {
    DISCO_OPT_ROOM_COV = 0,               // "room_cov": one-pass room kernel for the wide shapes (0: apply + staged covariance)
    DISCO_OPT_OVERLAP_SOLVES,           // "overlap_solves": whole-path calls run the batch as two halves on two streams
    DISCO_OPT_SOLVE_DPP,                // "solve_dpp": 9 <= P <= 16 solved in registers with DPP row broadcasts (k_solve_dpp.h; 0: the LDS group solver)
    DISCO_OPT_SOLVE_THREAD,             // "solve_thread": 5 <= P <= 8 solved one THREAD per pencil (k_solve_small.h at one wave per SIMD, AGPRs as the second register file) instead of the LDS group solver
    DISCO_OPT_FUSE_WIDE_ISTFT,          // "fuse_wide_istft": whole-path calls of the wide shapes (P > 8) end in ONE filter + iSTFT pass (k_apply_istft_wide) instead of disco_apply + disco_istft
    DISCO_OPT_ONLINE_SQ32,              // "online_sq32": the online mode's thread solves (P <= 7) square in packed float32 (k_solve_small.h); 0: float64 throughout
    DISCO_OPT_PACKED_X,                 // "packed_x": the fused route of disco_tango_enhance keeps its workspace X in line-aligned rows [T][F - 1][M], the Nyquist bin in the DC slot (0: the public [T][F][M])
    DISCO_N_OPTIONS
};
namespace disco_host {
struct OptionInfo {
    const char *key, *env;
    int def;
};
const OptionInfo* option_table();
}  // namespace disco_host

// workgroups for n logical items dealt over the XCDs by disco::xcd_item (common.h): the next multiple of N_XCD
namespace disco_host {
inline long long xcd_grid(long long n) { return (n + disco::N_XCD - 1) / disco::N_XCD * disco::N_XCD; }
}  // namespace disco_host

// a library-owned device allocation that only ever grows (disco_host::grow); freed by disco_destroy
struct DevBlock {
    void* p = nullptr;
    size_t bytes = 0;
};

// ---- the covariance partial sums a context holds between calls -----------------------------------------------------------------------
// Every covariance pass (k_stft_cov, k_cov*, k_cov_wide, k_step2_cov_fused, k_room_cov) leaves UNFINISHED sums -- per node and bin, `blocks`
// blocks of P (P + 1) / 2 float4 -- in one of two context-owned blocks, and two records say what is in them.  Nothing outside the functions
// declared below (api_partials.hip) touches the fields.
//   full, tail   The full block takes sums that hold the whole triangle.  The tail block takes step-2 sums that LACK their leading M x M
//                block, because the kept step-1 sums in the full block are that block (k_step2_cov_fused<.., true>, k_cov_split_lds<..,
//                true>, k_room_cov): one pass less over the M x M pairs, and the two must not share a block.
//   pending      what the last producer left for disco_gevd_mwf_r1_pending / cov_finalize: blocks (0 = nothing), P, and whether it
//                sits in the tail block.  Pending in the tail block implies kept step-1 sums in the full block.
//   kept step 1  the full block holds step-1 sums (P = M) of all nodes of every room, computed from the arrays X and mask: M (0 = it
//                does not), blocks, and the two arrays, whose IDENTITY is what grants a re-use (step1_held).
// What ends a record:
//   * a producer writing the full block ends the kept step-1 record (partials_commit) unless it re-establishes it (step1_keep);
//   * a block that has to GROW is freed: growing the full block forgets both records, growing the tail block drops only a pencil pending
//     in it -- the step-1 sums sit in the full block, and the caller has already decided its re-use from them (partials_begin).  So a
//     staged-API caller who makes a block grow between a covariance call and its solve gets "no covariance call has left partial sums",
//     not a solve of a fresh block;
//   * disco_set_tuning and disco_set_lengths forget both records (partials_forget): sums of another launch geometry or of other clip
//     lengths must neither be solved nor paired with;
//   * disco_set_node_shard drops the pending record only (pending_drop): the pending solve sizes its batch by the shard.  The kept step-1
//     record stays: it is only ever made with every node here, and every reader of it refuses under a shard.
struct Partials {
    DevBlock full, tail;
    int pend_blocks = 0, pend_P = 0;
    bool pend_tail = false;
    int loc_blocks = 0, loc_M = 0;
    const void *loc_X = nullptr, *loc_mask = nullptr;
};

struct disco_ctx {
    disco_cfg cfg{};
    int T = 0, F = 0;
    float* d_win = nullptr;
    c32* d_tw = nullptr;
    DevBlock own_ws;                 // workspace of the whole-path calls that are given none (ensure_own_ws)
    Partials partials;
    const void* ref_ws = nullptr;    // workspace in which a disco_tango_reference(steps = 1) call left its state for a steps = 2 call (else NULL)
    const void *ref_y = nullptr, *ref_s = nullptr, *ref_n = nullptr;   // ... and the inputs that state was computed from
    c32* d_tw_conv = nullptr;        // 1024-point twiddles of disco_rir_convolve (== d_tw when n_fft is 1024), lazy
    DevBlock conv_ws;                // its spectra workspace, lazy
    c32* src_tw[23] = {};            // twiddle tables of disco_noise_from_signal, one per n_fft = 2^p (api_sources.hip), lazy
    DevBlock src_ws;                 // its two complex planes, lazy
    int k0 = 0, Kl = 0;              // node shard: this context holds nodes [k0, k0 + Kl) of every room (default 0, K)
    int zblk = 0;                    // layout of the exchanged-signal arguments Zs / Zn / Z (disco_set_z_blocks; default K = plain)
    int tune_runw = 0, tune_cov_chunks = 0, tune_step2_chunks = 0, tune_pairs = 0;   // disco_set_tuning overrides (0 = batch-size heuristic)
    int opt[DISCO_N_OPTIONS] = {};   // disco_set_option values (DISCO_OPT_*)
    int n_cu = 0;                    // compute units of cfg.device (the persistent kernels start one workgroup per CU)
    int geom_rooms = 0;              // batch size the launch-geometry heuristics look at (cfg.rooms; a half-batch child: its parent's)
    // two half-batch children (rooms split [0, R/2) and [R/2, R)) + the second stream / events of the overlapped whole-path calls
    // (DISCO_OPT_OVERLAP_SOLVES): one half's solves run beside the other half's streaming kernels.  NULL when not in use.
    disco_ctx* half[2] = {nullptr, nullptr};
    disco_ctx* parent = nullptr;     // set in a child
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // per-stage hipEvent timers of the whole-path entry points (disco_stage_timing / disco_stage_report)
    struct StageRec {
        char name[32];
        std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
    };
    bool stage_on = false;
    std::vector<StageRec> stages;
    // per-room clip lengths (disco_set_lengths).  d_lens is what the kernels receive: NULL for the uniform batch, else cfg.rooms ints on
    // the device -- the context's own block (d_lens_own, allocated by the first disco_set_lengths and rewritten in place by later ones),
    // or, in a half-batch child, its slice of the parent's block.  h_lens is the host copy (empty = none).
    std::vector<int32_t> h_lens;
    int* d_lens = nullptr;
    int* d_lens_own = nullptr;
    char err[512] = "";
};

#define HIPCHK(ctx, call)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s", #call, hipGetErrorString(e_)); \
            return DISCO_E_HIP_BASE - (int)e_;                                                  \
        }                                                                                       \
    } while (0)

static inline int fail(disco_ctx* ctx, int code, const char* msg) {
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s", msg);
    return code;
}

static inline int check_launch(disco_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(ctx->err, sizeof(ctx->err), "launch of %s failed: %s", what, hipGetErrorString(e));
        return DISCO_E_HIP_BASE - (int)e;
    }
    return 0;
}

// Every entry point runs on the context's own device, whatever the calling thread's current device is, and leaves the
// caller's current device as it found it (two contexts on two GPUs in one process; a host such as torch switching devices).
struct DevGuard {
    int prev = -1;
    bool ok = true;
    explicit DevGuard(int device) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        if (cur != device) {
            ok = hipSetDevice(device) == hipSuccess;
            prev = cur;
        }
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard&) = delete;
    DevGuard& operator=(const DevGuard&) = delete;
};
// Entry points whose ctx may be NULL (the DNN's helpers and the training bank own no context): the launch then goes to the calling thread's
// current device, and a failed launch is reported by its code alone.
static inline int current_device(const disco_ctx* ctx) {
    if (ctx) return ctx->cfg.device;
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}
static inline int launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : DISCO_E_HIP_BASE - (int)e;
}
#define DISCO_ENTER(ctx)                                                                        \
    if (!(ctx)) return DISCO_E_ARG;                                                                  \
    DevGuard dev_guard_((ctx)->cfg.device);                                                          \
    if (!dev_guard_.ok) return fail((ctx), DISCO_E_HIP_BASE, "hipSetDevice(cfg.device) failed")

// ---- per-stage timers ---------------------------------------------------------------------------------------------------
// STAGE(ctx, s, "name", call): when disco_stage_timing(ctx, 1) is in force, brackets `call` (one or more launches on stream
// s) with two hipEvents recorded on that stream; otherwise just evaluates it.  Nothing is synchronised here.
static inline void stage_clear(disco_ctx* ctx) {
    for (auto& st : ctx->stages)
        for (auto& e : st.evs) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    ctx->stages.clear();
}
struct StageScope {
    disco_ctx* ctx;
    hipStream_t st;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const char* name;
    StageScope(disco_ctx* c, disco_stream s, const char* n) : ctx(c), st((hipStream_t)s), name(n) {
        if (!ctx->stage_on) return;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            e0 = e1 = nullptr;
            return;
        }
        (void)hipEventRecord(e0, st);
    }
    ~StageScope() {
        if (!e0) return;
        (void)hipEventRecord(e1, st);
        for (auto& r : ctx->stages)
            if (!strncmp(r.name, name, sizeof(r.name))) {
                r.evs.emplace_back(e0, e1);
                return;
            }
        disco_ctx::StageRec r;
        snprintf(r.name, sizeof(r.name), "%s", name);
        r.evs.emplace_back(e0, e1);
        ctx->stages.push_back(std::move(r));
    }
};
#define STAGE(ctx, s, name, call) ([&]() { StageScope stage_scope_((ctx), (s), (name)); return (call); }())

// entry points that do not take per-room lengths (the online mode, disco_mask_ivad, anything under a node shard) refuse while they are set
static inline bool has_lengths(const disco_ctx* ctx) { return ctx->d_lens != nullptr; }
#define DISCO_REFUSE_LENGTHS(ctx, who) \
    if (has_lengths(ctx)) return fail((ctx), DISCO_E_UNSUPPORTED, who ": per-room lengths are set (disco_set_lengths); not supported here")

// whole-path entry points work on all nodes of a room and on their own plain [R][K] exchanged-signal arrays
static inline bool sharded(const disco_ctx* ctx) { return ctx->Kl != ctx->cfg.nodes || ctx->zblk != ctx->cfg.nodes; }

// ---- the family: a context and its half-batch children ------------------------------------------------------------------------------
// Every walk over "this context and its children" goes through these two (the parent first), and what a child takes from its parent is
// stated once, in child_follow (api_core.hip).
template <class Ctx, class Fn>
inline void for_children(Ctx* ctx, Fn fn) {                // fn(child, h) for each child that exists
    for (int h = 0; h < 2; ++h)
        if (ctx->half[h]) fn(ctx->half[h], h);
}
template <class Ctx, class Fn>
inline void for_family(Ctx* ctx, Fn fn) {                  // fn(context): the parent, then its children
    fn(ctx);
    for_children(ctx, [&](auto* ch, int) { fn(ch); });
}
// first room of child h in its parent's batch: the rooms are split [0, R / 2) and [R / 2, R)
static inline int child_room0(const disco_ctx* parent, int h) { return h ? parent->cfg.rooms / 2 : 0; }
// a child's failure reported as the parent's: its message lifted, its code returned
static inline int lift_child_error(disco_ctx* ctx, const disco_ctx* child, int rc) { return fail(ctx, rc, child->err); }

namespace disco_host {
using disco::c32;
// the pieces of per-context state a child follows its parent in (child_follow)
enum { FOLLOW_TUNING = 1, FOLLOW_OPTIONS = 2, FOLLOW_STAGES = 4, FOLLOW_LENGTHS = 8, FOLLOW_ALL = 15 };
// child h takes the pieces `what` from its parent and drops what each invalidates (the definition says which)
void child_follow(const disco_ctx* parent, int h, int what);
// reserve_scratch for the context, then for its children
int reserve_family(disco_ctx* ctx);

struct WsLayout {
    size_t X, z, yf, Rss, Rnn, w, w2, total;
};
struct RefLayout {
    size_t Xy, Xs, Xn, zy, zs, zn_, znres, rows_s, rows_n, mz, mw, mc, Rss, Rnn, Rtmp, w_loc, w_glo, total;
};
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
// offsets of consecutive aligned arrays in a workspace: take(bytes) -> where the array starts; `o`: the total so far
struct Take {
    size_t o = 0;
    size_t operator()(size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes);
        return at;
    }
};
inline unsigned ew_grid(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 16384); }
// an element-wise kernel over n items: 256 threads per workgroup, grid-stride beyond 16384 workgroups
template <class Kernel, class... Args>
inline void ew_launch(Kernel k, long long n, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(k, dim3(ew_grid(n)), dim3(256), 0, st, args...);
}
WsLayout ws_layout(const disco_ctx* ctx);
RefLayout ref_layout(const disco_ctx* ctx);

// launch geometry (batch-size heuristics / disco_set_tuning)
int cov_chunks(const disco_ctx* ctx);
int room_chunks(const disco_ctx* ctx);
int cov1_f64_chunks(const disco_ctx* ctx);
int step2_chunks(const disco_ctx* ctx, int tiles_plus_1);
int stft_cov_chunks(const disco_ctx* ctx, int* runw_out);

// library-owned device memory (api_partials.hip)
int grow(disco_ctx* ctx, DevBlock& b, size_t need);       // no-op when large enough, else free + allocate: the contents are gone
int ensure_own_ws(disco_ctx* ctx, size_t bytes);          // ... of own_ws; a steps = 1 state of disco_tango_reference goes with the freed block
int reserve_scratch(disco_ctx* ctx);
// the partial sums (struct Partials above)
// What one covariance pass leaves: for each of G nodes and each bin, `blocks` blocks of P (P + 1) / 2 float4, in the full or the tail block.
// A producer builds its plan once, before its launch; the block is sized (partials_begin) and the record written (partials_commit) from
// that one value, and bytes() is the only place the size of such sums is written.
struct SumsPlan {
    long long G;         // nodes of the batch held by this context: rooms x Kl
    int chunks;          // frame chunks of the launch
    int blocks;          // blocks per node and bin: `chunks`, or two per chunk where the kernel hands over (hi, lo) pairs
    int P;
    bool tail;
    int pairs() const { return P * (P + 1) / 2; }
    size_t bytes(int F) const { return (size_t)G * blocks * F * pairs() * sizeof(float4); }
};
// a producer, before its launch: the block its plan names, large enough for it; NULL with *rc set when that fails
float4* partials_begin(disco_ctx* ctx, const SumsPlan& plan, int* rc);
// ... after it: what it left.  Sums in the full block end the kept step-1 record; a step-1 producer re-establishes it with step1_keep
void partials_commit(disco_ctx* ctx, const SumsPlan& plan);
void step1_keep(disco_ctx* ctx, const void* X, const void* mask);     // the sums just committed are step-1 sums of X with mask
bool step1_any(const disco_ctx* ctx);                                 // step-1 sums of this context's M are kept
bool step1_held(const disco_ctx* ctx, const void* X, const void* mask);   // ... and were computed from THESE arrays: the re-use guard
void pending_drop(disco_ctx* ctx);
void partials_forget(disco_ctx* ctx);
int partials_reserve(disco_ctx* ctx, size_t full_bytes, size_t tail_bytes);
size_t partials_bytes(const disco_ctx* ctx);
// what the pending record hands its readers: the blocks of the pencil and, when they lack the leading M_loc x M_loc block, the kept
// step-1 blocks that are it (else NULL, 0, 0).  false: nothing is pending
struct PendingSums {
    const float4* part;
    int blocks, P;
    const float4* part_loc;
    int blocks_loc, M_loc;
};
bool partials_pending(const disco_ctx* ctx, PendingSums* out);
// half-batch children of the overlapped whole-path calls: created when the batch is large enough (or the option forces it)
int ensure_halves(disco_ctx* ctx);
bool overlap_applies(const disco_ctx* ctx);
// the workspace of a whole-path call: the caller's if given (size-checked), else the context's own (grown on demand)
int locate_ws(disco_ctx* ctx, void* workspace, size_t workspace_bytes, size_t need, char** ws_out, const char* who);
// ... for a call that overwrites it: a steps = 1 state of disco_tango_reference kept in that workspace ends here
int acquire_ws(disco_ctx* ctx, void* workspace, size_t workspace_bytes, const WsLayout& l, char** ws_out, const char* who);

// transforms of signals of any length with the context's window / FFT size / padding (api_stft.hip)
// lens / sig_per_room: per-room clip lengths (device array, signal g belongs to room g / sig_per_room) or NULL
int stft_any(disco_ctx* ctx, const float* x, int64_t n_sig, int chans, disco_c32* X, int L, int T, disco_stream s, const int* lens = nullptr,
             int sig_per_room = 1);
int istft_any(disco_ctx* ctx, const disco_c32* Z, int64_t n_sig, float* out, int L, int T, disco_stream s, bool solo, const int* lens = nullptr,
              int sig_per_room = 1);
// per-room lengths and the n_sig of a stage call: signal g belongs to room g / (n_sig / rooms); 0, or an error code with the message set
int lengths_sig_per_room(disco_ctx* ctx, int64_t n_sig, const char* who, int* sig_per_room);

// stages (each leaves its partial sums pending in the context; see the definitions)
int cov_finalize(disco_ctx* ctx, disco_c32* Rss, disco_c32* Rnn, disco_stream s);      // of the pending sums (whole triangle, full block)
// the body of an entry point `who` that runs one covariance pass and hands out the matrices where asked: Rss and Rnn both or neither
// (`refusal`: the message where it is not the usual one), the pass -- its sums stay pending --, cov_finalize if they were given
template <class Pass>
inline int cov_pass_entry(disco_ctx* ctx, const char* who, disco_c32* Rss, disco_c32* Rnn, disco_stream s, Pass pass,
                          const char* refusal = nullptr) {
    if ((Rss == nullptr) != (Rnn == nullptr))
        return fail(ctx, DISCO_E_ARG, refusal ? refusal : (std::string(who) + ": Rss and Rnn must both be given or both be NULL").c_str());
    const int rc = pass();
    if (rc || !Rss) return rc;
    return cov_finalize(ctx, Rss, Rnn, s);
}
int cov_partials(disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* Zs, const disco_c32* Zn, int mask_remote, int P,
                 disco_stream s, bool skiploc = false);
bool room_cov_ok(const disco_ctx* ctx, const disco_c32* X, const float* mask);
int room_cov_partials(disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* w_loc, disco_c32* z, disco_stream s,
                      bool store_z = true);
// exchange + step-2 statistics with z materialised (api_path.hip): the room pass where the shape and the context's state allow it, else
// disco_apply + cov_partials.  The one body behind the whole-path calls and disco_selftest_staged_step2.  route_out (may be NULL): which
// of DISCO_STAGED_ROUTE_* ran
int staged_step2(disco_ctx* ctx, const disco_c32* X, const float* mask_w, bool same_mask, const disco_c32* w_loc, disco_c32* z, bool store_z,
                 disco_stream s, int* route_out = nullptr);
// cov_finalize for whatever is pending, a pencil left as tail blocks + kept step-1 blocks included (disco_selftest_pending_matrices)
int pending_matrices(disco_ctx* ctx, disco_c32* Rss, disco_c32* Rnn, disco_stream s);
// rows of X: the public [T][F][M], or the packed workspace layout [T][F - 1][M] with the Nyquist bin in the DC slot (k_stft.h; 512 points)
enum class XLayout { Public, Packed };
// leading M x M block of the step-2 sums: accumulated with the rest, or step 1's -- the caller has checked that the step-1 partial sums of
// THIS X with THIS mask are still kept (step1_held); the block is then neither accumulated nor written and the sums go to the tail block
enum class LeadBlock { Accumulate, Step1 };
// store = false (single-node path): the spectra are not written (X may be NULL); only for shapes the fused kernel takes
// zero_beyond = false (per-room lengths): the frames of X beyond a room's clip are left unwritten -- only for a caller whose every reader of
// X knows the lengths (the fused route of disco_tango_enhance)
// layout = Packed: needs stored spectra -- the same partial sums
struct StftCovOpts {
    bool store = true, zero_beyond = true;
    XLayout layout = XLayout::Public;
};
int stft_cov_partials(disco_ctx* ctx, const float* y, const float* mask_z, disco_c32* X, disco_stream s, const StftCovOpts& o = {});
int step2_cov_partials(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc, disco_c32* z_out, disco_stream s,
                       LeadBlock lead, XLayout layout);
// filter + iSTFT of the fused route (disco_step2_apply_istft_fused)
int step2_apply_istft(disco_ctx* ctx, const disco_c32* X, const disco_c32* w_loc, const disco_c32* w_glo, float* out, disco_stream s,
                      XLayout layout);
int stft_apply_istft(disco_ctx* ctx, const float* y, const disco_c32* w, float* out, disco_stream s);
bool step2_apply_istft_ok(const disco_ctx* ctx);
bool apply_istft_wide_ok(const disco_ctx* ctx);
int apply_istft_wide(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const disco_c32* w, disco_c32* yf, float* out, disco_stream s);
}  // namespace disco_host
