// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): whole-path entry points
#include "host.h"

#include <functional>
#include "k_apply.h"
#include "k_cov.h"
#include "k_cov_wide.h"
#include "k_stft.h"

using namespace disco;
using namespace disco_host;

// ---------------------------------------------------------------------------------------------------------
// whole path
// ---------------------------------------------------------------------------------------------------------
// where child h's slice of an overlapped call's workspace starts: child 1's behind child 0's
static size_t child_ws_offset(const disco_ctx* ctx, int h) { return h ? align_up(ws_layout(ctx->half[0]).total) : 0; }

namespace disco_host {
WsLayout ws_layout(const disco_ctx* ctx) {
    const disco_cfg& c = ctx->cfg;
    const size_t G = (size_t)c.rooms * c.nodes, TF = (size_t)ctx->T * ctx->F;
    const size_t Pmax = (size_t)c.mics + c.nodes - 1;
    WsLayout l;
    Take take;
    l.X = take(G * TF * c.mics * sizeof(c32));
    l.z = take(G * TF * sizeof(c32));
    l.yf = take(G * TF * sizeof(c32));
    l.Rss = take(G * ctx->F * Pmax * Pmax * sizeof(c32));
    l.Rnn = take(G * ctx->F * Pmax * Pmax * sizeof(c32));
    l.w = take(G * ctx->F * Pmax * sizeof(c32));
    l.w2 = take(G * ctx->F * Pmax * sizeof(c32));
    l.total = take.o;
    // an overlapped call hands each half-batch child its own slice (child_args): the two slices must fit
    if (ctx->half[0] && ctx->half[1]) l.total = std::max(l.total, child_ws_offset(ctx, 1) + ws_layout(ctx->half[1]).total);
    return l;
}
}  // namespace disco_host

// ---- a whole-path call as a list of steps -----------------------------------------------------------------------------------
// Every whole-path entry point builds the list of its stages (one kernel family each) and runs it: in order on the caller's stream,
// or -- the overlapped forms, DISCO_OPT_OVERLAP_SOLVES -- over the two half-batch children:
//   1 / 2 (default / forced)  child A entirely on the caller's stream, child B entirely on the side stream: the two sequences drift
//         against each other, so a solve -- a compute kernel that moves almost no data -- mostly meets a streaming kernel of the other
//         half, and each half's kernel tails are filled by the other half.  Measured on C3: 19.67 -> 19.14 ms.
// (Round 3 also built a software-pipelined order -- streaming kernels on the caller's stream, only the solves on the side stream: every solve
// hidden, but two half-batch launches of a streaming kernel cost more than one whole-batch launch, C3 18.99 -> 19.29 ms; removed in round 5.)
// Nothing synchronises with the host, and the side stream is forked from / joined to the caller's, so the sequence can still be captured
// into one hipGraph.
namespace {
struct Step {
    const char* name;                          // stage name for the timers; nullptr: the callee brackets its own stages
    bool side;                                 // a solve: runs on the side stream of an overlapped call
    std::function<int(disco_stream)> run;
};
using Steps = std::vector<Step>;

int run_step(disco_ctx* ctx, Step& x, disco_stream st) { return x.name ? STAGE(ctx, st, x.name, x.run(st)) : x.run(st); }

int run_steps(disco_ctx* ctx, Steps& steps, disco_stream s) {
    for (auto& x : steps) {
        const int rc = run_step(ctx, x, s);
        if (rc) return rc;
    }
    return 0;
}

int run_pipelined(disco_ctx* ctx, Steps (&steps)[2], disco_stream s) {
    hipStream_t s0 = (hipStream_t)s, s1 = ctx->side_stream;
    const size_t n = steps[0].size();
    if (steps[1].size() != n) return fail(ctx, DISCO_E_ARG, "overlapped call: step lists do not match");
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, s0));
    HIPCHK(ctx, hipStreamWaitEvent(s1, ctx->ev_fork, 0));
    int rc = 0;
    // one child per stream.  A failure inside the loop is collected, not returned: the join below must be reached whatever happened, or the
    // caller's stream stays forked (and a capture unjoined)
    for (int h = 0; h < 2 && !rc; ++h)
        for (size_t i = 0; i < n && !rc; ++i) {
            rc = run_step(ctx->half[h], steps[h][i], (disco_stream)(h ? s1 : s0));
            if (rc) lift_child_error(ctx, ctx->half[h], rc);
        }
    const hipError_t e1 = hipEventRecord(ctx->ev_join, s1), e2 = hipStreamWaitEvent(s0, ctx->ev_join, 0);       // the join, whatever happened above
    if (!rc && (e1 != hipSuccess || e2 != hipSuccess)) {
        snprintf(ctx->err, sizeof(ctx->err), "joining the side stream failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        rc = DISCO_E_HIP_BASE - (int)(e1 != hipSuccess ? e1 : e2);
    }
    return rc;
}

// arguments of one (half-)batch of a whole-path call
struct PathArgs {
    const float *y, *mask_z, *mask_w;
    float* out;
    disco_c32 *z_y, *yf;
    char* ws;
};
// the slice of the caller's arrays / workspace that child h (rooms [r0, r0 + rooms_h)) works on
PathArgs child_args(const disco_ctx* ctx, const PathArgs& a, int h) {
    const disco_cfg& c = ctx->cfg;
    const size_t r0 = (size_t)child_room0(ctx, h);
    const size_t K = c.nodes, TF = (size_t)ctx->T * ctx->F, sy = K * c.mics * c.length, sm = K * TF, so = K * c.length;
    PathArgs b;
    b.y = a.y + r0 * sy;
    b.mask_z = a.mask_z + r0 * sm;
    b.mask_w = a.mask_w == a.mask_z ? b.mask_z : a.mask_w + r0 * sm;
    b.out = a.out + r0 * so;
    b.z_y = a.z_y ? a.z_y + r0 * sm : nullptr;
    b.yf = a.yf ? a.yf + r0 * sm : nullptr;
    b.ws = a.ws + child_ws_offset(ctx, h);
    return b;
}

// the arrays of one (half-)batch of a whole-path call: X, w, w2 in this context's workspace; z and the filtered spectra yo in the
// caller's z_y / yf where given, else in the workspace too
struct PathBufs {
    disco_c32 *X, *z, *yo, *w, *w2;
};
PathBufs path_bufs(const disco_ctx* ctx, const PathArgs& a) {
    const WsLayout l = ws_layout(ctx);
    auto at = [&](size_t off) { return (disco_c32*)(a.ws + off); };
    return {at(l.X), a.z_y ? a.z_y : at(l.z), a.yf ? a.yf : at(l.yf), at(l.w), at(l.w2)};
}
}  // namespace

extern "C" size_t disco_workspace_bytes(const disco_ctx* ctx) { return ctx ? ws_layout(ctx).total : 0; }

namespace disco_host {
// caller's workspace if given (size-checked), else the context's own (grown on demand)
int locate_ws(disco_ctx* ctx, void* workspace, size_t workspace_bytes, size_t need, char** ws_out, const char* who) {
    if (workspace) {
        if (workspace_bytes < need) return fail(ctx, DISCO_E_ARG, (std::string(who) + ": workspace too small").c_str());
        *ws_out = (char*)workspace;
        return 0;
    }
    const int rc = ensure_own_ws(ctx, need);
    *ws_out = (char*)ctx->own_ws.p;
    return rc;
}
int acquire_ws(disco_ctx* ctx, void* workspace, size_t workspace_bytes, const WsLayout& l, char** ws_out, const char* who) {
    const int rc = locate_ws(ctx, workspace, workspace_bytes, l.total, ws_out, who);
    if (!rc && ctx->ref_ws == *ws_out) ctx->ref_ws = nullptr;      // a steps = 1 state of disco_tango_reference in this workspace is overwritten
    return rc;
}
}  // namespace disco_host

// step 2 on the on-chip z exchange: whenever all nodes of a room share the GPU and P <= 8, unless the context asks for the staged form
static bool fused_route(const disco_ctx* ctx) {
    const disco_cfg& c = ctx->cfg;
    return c.nodes > 1 && c.mics + c.nodes - 1 <= 8 && !(c.flags & DISCO_FLAG_STAGED_STEP2);
}
// ... and it ends in ONE filter + iSTFT pass, yf staying on chip: yf not asked for, 512 points, a shape the kernel takes.  Decides the tail
// of disco_tango_enhance, and with it what may be left out of X and the layout of its rows (enhance_steps)
static bool fused_tail_one_pass(const disco_ctx* ctx, const disco_c32* yf) {
    return fused_route(ctx) && !yf && ctx->cfg.n_fft == 512 && step2_apply_istft_ok(ctx);
}

// exchange + step-2 statistics with z materialised, mask_for_z = 'local': ONE pass over X for every node of a room where the shape and the
// context's state allow it (k_room_cov), else the filter pass followed by the covariance pass that reads X again and the K - 1 remote z's
namespace disco_host {
int staged_step2(disco_ctx* ctx, const disco_c32* X, const float* mask_w, bool same_mask, const disco_c32* w_loc, disco_c32* z, bool store_z,
                 disco_stream s, int* route_out) {
    const disco_cfg& c = ctx->cfg;
    if (same_mask && room_cov_ok(ctx, X, mask_w)) {
        if (route_out) *route_out = DISCO_STAGED_ROUTE_ROOM;
        return STAGE(ctx, s, "room_cov2", room_cov_partials(ctx, X, mask_w, w_loc, z, s, store_z));
    }
    int rc = STAGE(ctx, s, "apply1", disco_apply(ctx, X, nullptr, w_loc, c.mics, 1, z, s));
    if (rc) return rc;
    const disco_c32* zr = c.nodes > 1 ? z : nullptr;
    rc = STAGE(ctx, s, "cov2", cov_partials(ctx, X, mask_w, zr, zr, 1, c.mics + c.nodes - 1, s, same_mask && c.nodes > 1));
    if (route_out) {                           // the step-1 block was skipped <=> the pencil is pending as tail blocks + the kept step-1 blocks
        PendingSums ps;
        *route_out = !rc && partials_pending(ctx, &ps) && ps.part_loc ? DISCO_STAGED_ROUTE_SPLIT_SKIPLOC : DISCO_STAGED_ROUTE_WHOLE;
    }
    return rc;
}
}  // namespace disco_host

static void push_staged_step2(disco_ctx* ctx, Steps& st, const disco_c32* X, const float* mask_w, bool same_mask, const disco_c32* w_loc,
                              disco_c32* z, bool store_z) {
    st.push_back({nullptr, false, [=](disco_stream s) { return staged_step2(ctx, X, mask_w, same_mask, w_loc, z, store_z, s); }});
}

// test-only (include/disco_hip.h): step 1 on the caller's spectra, then the staged step 2 of the whole-path calls with the same mask
extern "C" int disco_selftest_staged_step2(disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* w_loc, disco_c32* z,
                                           int store_z, int* route_out, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!X || !mask || !w_loc || !z) return fail(ctx, DISCO_E_ARG, "disco_selftest_staged_step2: null argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_selftest_staged_step2: node shard active");
    if (route_out) *route_out = 0;
    const int rc = cov_partials(ctx, X, mask, nullptr, nullptr, 1, ctx->cfg.mics, s);      // keeps the step-1 record of X / mask
    if (rc) return rc;
    return staged_step2(ctx, X, mask, true, w_loc, z, store_z != 0, s, route_out);
}

// the global filter + iSTFT: wide shapes in one pass, yf stays on chip (and goes out only when the caller asked for it: yf may be NULL)
static void push_apply2_istft(disco_ctx* ctx, Steps& st, const disco_c32* X, const disco_c32* z, const disco_c32* w, disco_c32* yf,
                              disco_c32* yo, float* out) {
    const disco_cfg& c = ctx->cfg;
    const int64_t G = (int64_t)c.rooms * c.nodes;
    const int P2 = c.mics + c.nodes - 1;
    if (c.nodes > 1 && apply_istft_wide_ok(ctx)) {
        st.push_back({"apply2_istft", false, [=](disco_stream s) { return apply_istft_wide(ctx, X, z, w, yf, out, s); }});
        return;
    }
    st.push_back({"apply2", false, [=](disco_stream s) { return disco_apply(ctx, X, c.nodes > 1 ? z : nullptr, w, P2, 1, yo, s); }});
    st.push_back({"istft", false, [=](disco_stream s) { return disco_istft(ctx, yo, G, out, s); }});
}

// a whole-path call: one list of steps on the caller's stream, or -- `overlap` and the half-batch children exist -- one list per child
static int run_path(disco_ctx* ctx, const PathArgs& a, bool overlap, const std::function<void(disco_ctx*, const PathArgs&, Steps&)>& build,
                    disco_stream s) {
    if (overlap && overlap_applies(ctx) && ctx->half[0] && ctx->half[1]) {
        Steps st[2];
        for (int h = 0; h < 2; ++h) build(ctx->half[h], child_args(ctx, a, h), st[h]);
        return run_pipelined(ctx, st, s);
    }
    Steps st;
    build(ctx, a, st);
    return run_steps(ctx, st, s);
}

// offline_tango's y branch as a list of steps (tango.py:326-450 + 528); `a` names this context's slice of the batch
static void enhance_steps(disco_ctx* ctx, const PathArgs& a, Steps& st) {
    const disco_cfg& c = ctx->cfg;
    const float *y = a.y, *mask_z = a.mask_z, *mask_w = a.mask_w;
    float* out = a.out;
    disco_c32 *z_y = a.z_y, *yf = a.yf;
    const PathBufs b = path_bufs(ctx, a);
    disco_c32 *X = b.X, *z = b.z, *yo = b.yo, *w = b.w, *w2 = b.w2;      // (named: the step lambdas capture them by value)
    const int64_t G = (int64_t)c.rooms * c.nodes;
    const int M = c.mics;
    const bool same_mask = mask_w == mask_z;
    auto solve_pending = [ctx](disco_c32* w_out) { return [ctx, w_out](disco_stream s) { return disco_gevd_mwf_r1_pending(ctx, ctx->cfg.mu, w_out, nullptr, s); }; };

    if (c.nodes == 1 && same_mask && !z_y && !yf && c.n_fft == 512 && M <= 4) {
        // single node, enhanced output only (config C2): nothing is materialised -- one pass over the samples for the
        // statistics, one for filter + iSTFT with the spectra recomputed (get_z_signals.py:274-315 + tango.py:528)
        StftCovOpts no_spectra;
        no_spectra.store = false;
        st.push_back({nullptr, false, [=](disco_stream s) { return stft_cov_partials(ctx, y, mask_z, nullptr, s, no_spectra); }});
        st.push_back({"solve1", true, solve_pending(w)});
        st.push_back({"stft_apply_istft", false, [=](disco_stream s) { return stft_apply_istft(ctx, y, w, out, s); }});
        return;
    }
    // step 1 (tango.py:326-376): STFT + covariance in one pass, solve straight from the partial sums
    // per-room lengths: both readers of X on the fused route without yf (k_step2_cov_fused, k_step2_apply_istft) stop at a room's own
    // frames, so the frames of X beyond them need not be written; every other route reads them and finds the zeros it relies on
    const bool one_pass_tail = fused_tail_one_pass(ctx, yf);
    const bool x_zeros = !one_pass_tail;
    // ... and on that branch X never leaves the workspace, so its rows may take the packed layout ("packed_x", k_stft.h k_stft_cov: [T][F - 1][M],
    // the Nyquist bin in the DC slot): every wave load and store of the three passes over X then covers whole 128-byte lines.  The slot of
    // X in the workspace keeps its size (the packed array is 1 / F smaller), so one workspace serves both values of the option.
    const XLayout layout = one_pass_tail && ctx->opt[DISCO_OPT_PACKED_X] != 0 ? XLayout::Packed : XLayout::Public;
    StftCovOpts step1;
    step1.zero_beyond = x_zeros;
    step1.layout = layout;
    st.push_back({nullptr, false, [=](disco_stream s) { return stft_cov_partials(ctx, y, mask_z, X, s, step1); }});
    st.push_back({"solve1", true, solve_pending(w)});

    if (fused_route(ctx)) {
        // same mask array in both steps (oracle masks; a DNN mask re-used, tango.py:388-389): the leading M x M block of the
        // step-2 covariances IS the step-1 covariance still held as partial sums -> not recomputed
        st.push_back({"step2_cov", false, [=](disco_stream s) {
            return step2_cov_partials(ctx, X, mask_w, w, z_y, s, step1_held(ctx, X, mask_w) ? LeadBlock::Step1 : LeadBlock::Accumulate, layout);
        }});
        st.push_back({"solve2", true, solve_pending(w2)});
        if (one_pass_tail) {
            st.push_back({"step2_apply_istft", false, [=](disco_stream s) { return step2_apply_istft(ctx, X, w, w2, out, s, layout); }});
            return;
        }
        st.push_back({"step2_apply", false, [=](disco_stream s) { return disco_step2_apply_fused(ctx, X, w, w2, nullptr, yo, s); }});
        st.push_back({"istft", false, [=](disco_stream s) { return disco_istft(ctx, yo, G, out, s); }});
        return;
    }
    if (c.nodes == 1 && same_mask) {
        if (!z_y && !yf && step2_apply_istft_ok(ctx)) {
            // single node, enhanced output only: filter + iSTFT in one pass over X, z never reaches HBM
            st.push_back({"step2_apply_istft", false, [=](disco_stream s) { return disco_step2_apply_istft_fused(ctx, X, w, w, out, s); }});
            return;
        }
        // single node, same mask: step 2 would rebuild the very same statistics from the very same inputs
        // (P = M, nothing to append), so w_glo == w_loc and yf == z_y bit for bit (config C2).
        st.push_back({"apply1", false, [=](disco_stream s) { return disco_apply(ctx, X, nullptr, w, M, 1, z, s); }});
        st.push_back({"istft", false, [=](disco_stream s) {
            if (yf) HIPCHK(ctx, hipMemcpyAsync(yf, z, (size_t)G * ctx->T * ctx->F * sizeof(c32), hipMemcpyDeviceToDevice, (hipStream_t)s));
            return disco_istft(ctx, z, G, out, s);
        }});
        return;
    }
    // exchange + step 2 (tango.py:378-450) with z materialised
    push_staged_step2(ctx, st, X, mask_w, same_mask, w, z, true);
    st.push_back({"solve2", true, solve_pending(w)});
    push_apply2_istft(ctx, st, X, z, w, yf, yo, out);
}

extern "C" int disco_tango_enhance(disco_ctx* ctx, const float* y, const float* mask_z, const float* mask_w, float* out,
                                   disco_c32* z_y, disco_c32* yf, void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!y || !mask_z || !mask_w || !out) return fail(ctx, DISCO_E_ARG, "disco_tango_enhance: null argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_enhance: node shard active, drive the staged calls around an all-gather of z");
    const WsLayout l = ws_layout(ctx);
    char* ws = nullptr;
    int rcw = acquire_ws(ctx, workspace, workspace_bytes, l, &ws, "disco_tango_enhance");
    if (rcw) return rcw;
    const PathArgs a{y, mask_z, mask_w, out, z_y, yf, ws};
    // by default only where it was measured to pay: the fused route (C3: 19.67 -> 19.14 ms); forced (2 / 3) for every route
    return run_path(ctx, a, fused_route(ctx) || ctx->opt[DISCO_OPT_OVERLAP_SOLVES] >= 2, enhance_steps, s);
}

// ---- reference outputs: all nine returns of offline_tango, device resident ------------------------------------------------
namespace disco_host {
RefLayout ref_layout(const disco_ctx* ctx) {
    const disco_cfg& c = ctx->cfg;
    const size_t G = (size_t)c.rooms * c.nodes, TF = (size_t)ctx->T * ctx->F;
    const size_t Pmax = (size_t)c.mics + c.nodes - 1;
    RefLayout l;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes); return at; };
    l.Xy = take(G * TF * c.mics * sizeof(c32));
    l.Xs = take(G * TF * c.mics * sizeof(c32));
    l.Xn = take(G * TF * c.mics * sizeof(c32));
    l.zy = take(G * TF * sizeof(c32));
    l.zs = take(G * TF * sizeof(c32));
    l.zn_ = take(G * TF * sizeof(c32));
    l.znres = take(G * TF * sizeof(c32));
    l.rows_s = take(G * TF * sizeof(c32));
    l.rows_n = take(G * TF * sizeof(c32));
    l.mz = take(G * TF * sizeof(float));
    l.mw = take(G * TF * sizeof(float));
    l.mc = take(G * TF * sizeof(float));
    l.Rss = take(G * ctx->F * c.mics * c.mics * sizeof(c32));
    l.Rnn = take(G * ctx->F * c.mics * c.mics * sizeof(c32));
    l.Rtmp = take(G * ctx->F * c.mics * c.mics * sizeof(c32));
    l.w_loc = take(G * ctx->F * c.mics * sizeof(c32));
    l.w_glo = take(G * ctx->F * Pmax * sizeof(c32));
    l.total = o;
    return l;
}
}  // namespace disco_host

extern "C" size_t disco_reference_workspace_bytes(const disco_ctx* ctx) { return ctx ? ref_layout(ctx).total : 0; }

extern "C" size_t disco_owned_bytes(const disco_ctx* ctx) {
    size_t n = 0;
    if (ctx) for_family(ctx, [&n](const disco_ctx* x) { n += partials_bytes(x) + x->own_ws.bytes + x->conv_ws.bytes + x->src_ws.bytes; });
    return n;
}

extern "C" int disco_reserve(disco_ctx* ctx, int own_workspace) {
    DISCO_ENTER(ctx);
    if (own_workspace < 0 || own_workspace > 2) return fail(ctx, DISCO_E_ARG, "disco_reserve: own_workspace must be 0, 1 or 2");
    const int rc = reserve_family(ctx);
    if (rc || !own_workspace) return rc;
    size_t need = ws_layout(ctx).total;
    if (own_workspace == 2) need = std::max(need, ref_layout(ctx).total);
    return ensure_own_ws(ctx, need);
}

extern "C" int disco_tango_reference(disco_ctx* ctx, const float* y, const float* s_img, const float* n_img, const float* mask_z_in,
                                     const float* mask_w_in, int mask_for_z, int steps, const disco_ref_outputs* out,
                                     void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!y || !s_img || !n_img || !out) return fail(ctx, DISCO_E_ARG, "disco_tango_reference: null argument");
    if (steps < 1 || steps > 3) return fail(ctx, DISCO_E_ARG, "disco_tango_reference: steps must be 1, 2 or 3");
    if (mask_for_z < DISCO_MZ_LOCAL || mask_for_z > DISCO_MZ_PREVIOUS) return fail(ctx, DISCO_E_ARG, "disco_tango_reference: unknown mask_for_z");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_reference: node shard active");
    const disco_cfg& c = ctx->cfg;
    if (c.mask_type < DISCO_MASK_IRM || c.mask_type > DISCO_MASK_IAM) return fail(ctx, DISCO_E_ARG, "disco_tango_reference: unknown mask type");
    const int M = c.mics, K = c.nodes, P2 = M + K - 1;
    if (P2 > CW_PMAX || M > 8) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_reference: M + K - 1 > 32 or M > 8 not supported");
    // the workspace: the caller's, or a context-owned one kept in `own_ws` (shared with the enhanced-output entry points)
    // (located, not acquired: a steps = 2 call continues from the state in it, which is checked first and ends below)
    const RefLayout l = ref_layout(ctx);
    if (!workspace && ctx->own_ws.bytes < l.total && steps == 2)
        return fail(ctx, DISCO_E_ARG, "disco_tango_reference: steps = 2 needs the workspace of the preceding steps = 1 call");
    char* ws = nullptr;
    const int rcw = locate_ws(ctx, workspace, workspace_bytes, l.total, &ws, "disco_tango_reference");
    if (rcw) return rcw;
    if (steps == 2 && !(ctx->ref_ws == ws && ctx->ref_y == y && ctx->ref_s == s_img && ctx->ref_n == n_img))
        return fail(ctx, DISCO_E_ARG, "disco_tango_reference: steps = 2 needs the state a steps = 1 call with the same y, s, n left in the same "
                                      "workspace (no other whole-path call in between)");
    ctx->ref_ws = nullptr;
    hipStream_t st = (hipStream_t)s;
    const int64_t G = (int64_t)c.rooms * K;
    const long long nTF = (long long)G * ctx->T * ctx->F;
    const size_t plane_b = (size_t)nTF * sizeof(c32), mask_b = (size_t)nTF * sizeof(float);
    disco_c32 *Xy = (disco_c32*)(ws + l.Xy), *Xs = (disco_c32*)(ws + l.Xs), *Xn = (disco_c32*)(ws + l.Xn);
    disco_c32 *zy = (disco_c32*)(ws + l.zy), *zs = (disco_c32*)(ws + l.zs), *zn_ = (disco_c32*)(ws + l.zn_), *znres = (disco_c32*)(ws + l.znres);
    disco_c32 *rows_s = (disco_c32*)(ws + l.rows_s), *rows_n = (disco_c32*)(ws + l.rows_n);
    float *mz = (float*)(ws + l.mz), *mw = (float*)(ws + l.mw), *mc = (float*)(ws + l.mc);
    disco_c32 *Rss = (disco_c32*)(ws + l.Rss), *Rnn = (disco_c32*)(ws + l.Rnn), *Rtmp = (disco_c32*)(ws + l.Rtmp), *w_loc = (disco_c32*)(ws + l.w_loc), *w_glo = (disco_c32*)(ws + l.w_glo);
    const float thr = powf(10.f, c.mask_bin_thr_db / 10.f);
    const bool oracle_sigs = mask_for_z == DISCO_MZ_ORACLE_REFS || mask_for_z == DISCO_MZ_ORACLE_ZS;     // tango.py:343
    auto give = [&](void* dst, const void* src, size_t bytes) -> int {
        if (dst && dst != src) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    int rc;
    if (steps & 1) {
        // ---- STFTs of the mixture and of both images (tango.py:335-337)
        if ((rc = disco_stft(ctx, y, G, M, Xy, s))) return rc;
        if ((rc = disco_stft(ctx, s_img, G, M, Xs, s))) return rc;
        if ((rc = disco_stft(ctx, n_img, G, M, Xn, s))) return rc;
        // ---- step-1 mask at the reference microphone (tango.py:338-342)
        if (mask_z_in) {
            HIPCHK(ctx, hipMemcpyAsync(mz, mask_z_in, mask_b, hipMemcpyDeviceToDevice, st));
        } else {
            ew_launch(k_tf_mask_channel, nTF, st, (const c32*)Xs, (const c32*)Xn, mz, nTF, M, c.ref_mic, c.mask_type, c.mask_pow, thr, ctx->d_lens, ctx->T, ctx->F, K);
            if ((rc = check_launch(ctx, "k_tf_mask_channel"))) return rc;
        }
        // ---- step 1: local statistics, filter, compressed signals (tango.py:343-376)
        if (oracle_sigs) {            // s_hat = S, n_hat = N: Rss from the target image alone, Rnn from the noise image alone
            ew_launch(k_fill_f32, nTF, st, mc, 1.f, nTF);
            if ((rc = disco_cov_masked(ctx, Xs, mc, nullptr, nullptr, 0, M, Rss, Rtmp, s))) return rc;      // mask 1: Rss = <S S^H>  (Rtmp = 0)
            ew_launch(k_fill_f32, nTF, st, mc, 0.f, nTF);
            if ((rc = disco_cov_masked(ctx, Xn, mc, nullptr, nullptr, 0, M, Rtmp, Rnn, s))) return rc;      // mask 0: Rnn = <N N^H>  (Rtmp = 0)
            if ((rc = disco_gevd_mwf_r1(ctx, Rss, Rnn, G * ctx->F, M, c.mu, w_loc, nullptr, s))) return rc;
        } else {
            if ((rc = cov_partials(ctx, Xy, mz, nullptr, nullptr, 0, M, s))) return rc;
            if ((rc = disco_gevd_mwf_r1_pending(ctx, c.mu, w_loc, nullptr, s))) return rc;
        }
        if ((rc = disco_apply(ctx, Xy, nullptr, w_loc, M, 1, zy, s))) return rc;
        if ((rc = disco_apply(ctx, Xs, nullptr, w_loc, M, 1, zs, s))) return rc;
        if ((rc = disco_apply(ctx, Xn, nullptr, w_loc, M, 1, zn_, s))) return rc;
        if ((rc = disco_noise_residual(ctx, Xy, zy, znres, s))) return rc;                                  // tango.py:376
        if ((rc = give(out->z_y, zy, plane_b)) || (rc = give(out->z_s, zs, plane_b)) || (rc = give(out->z_n, zn_, plane_b)) ||
            (rc = give(out->zn, znres, plane_b)) || (rc = give(out->masks_z, mz, mask_b)))
            return rc;
        if (steps == 1) {               // the state a later steps = 2 call continues from
            ctx->ref_ws = ws;
            ctx->ref_y = y;
            ctx->ref_s = s_img;
            ctx->ref_n = n_img;
        }
    }
    if (!(steps & 2)) return 0;
    // ---- step-2 mask at channel 0 (tango.py:388-394)
    if (mask_w_in) {
        HIPCHK(ctx, hipMemcpyAsync(mw, mask_w_in, mask_b, hipMemcpyDeviceToDevice, st));
    } else {
        ew_launch(k_tf_mask_channel, nTF, st, (const c32*)Xs, (const c32*)Xn, mw, nTF, M, 0, c.mask_type, c.mask_pow, thr, ctx->d_lens, ctx->T, ctx->F, K);
        if ((rc = check_launch(ctx, "k_tf_mask_channel"))) return rc;
    }
    if ((rc = give(out->mask_w, mw, mask_b))) return rc;
    // ---- the exchanged rows (tango.py:396-429) and the global statistics (433-440)
    const disco_c32 *Zs_rows = zy, *Zn_rows = zy;
    int mask_remote = 0;
    if (K > 1) {
        switch (mask_for_z) {
            case DISCO_MZ_LOCAL: mask_remote = 1; break;
            case DISCO_MZ_NONE: Zn_rows = znres; break;
            case DISCO_MZ_DISTANT:
                ew_launch(k_mask_rows, nTF, st, (const c32*)zy, (const float*)mw, (c32*)rows_s, (c32*)rows_n, nTF);
                Zs_rows = rows_s;
                Zn_rows = rows_n;
                break;
            case DISCO_MZ_COMPRESSED: {           // the sender's mask from ITS compressed target / noise (get_mask(z_s, z_n), tango.py:402-403)
                ew_launch(k_tf_mask, nTF, st, (const c32*)zs, (const c32*)zn_, mc, nTF, c.mask_type, c.mask_pow, thr, ctx->d_lens, ctx->T, ctx->F, K);
                ew_launch(k_mask_rows, nTF, st, (const c32*)zy, (const float*)mc, (c32*)rows_s, (c32*)rows_n, nTF);
                Zs_rows = rows_s;
                Zn_rows = rows_n;
            } break;
            case DISCO_MZ_ORACLE_REFS:
                ew_launch(k_pick_channel, nTF, st, (const c32*)Xs, (c32*)rows_s, nTF, M, c.ref_mic);
                ew_launch(k_pick_channel, nTF, st, (const c32*)Xn, (c32*)rows_n, nTF, M, c.ref_mic);
                Zs_rows = rows_s;
                Zn_rows = rows_n;
                break;
            case DISCO_MZ_ORACLE_ZS: Zs_rows = zs; Zn_rows = zn_; break;
            default: break;                   // 'previous': unmasked z_y in both
        }
        if ((rc = check_launch(ctx, "reference rows"))) return rc;
    }
    if ((rc = cov_partials(ctx, Xy, mw, K > 1 ? Zs_rows : nullptr, K > 1 ? Zn_rows : nullptr, mask_remote, P2, s))) return rc;
    if ((rc = disco_gevd_mwf_r1_pending(ctx, c.mu, w_glo, nullptr, s))) return rc;
    // ---- the global filter on the mixture and on both images (tango.py:445-450); outputs straight into the caller's arrays
    if (out->yf && (rc = disco_apply(ctx, Xy, K > 1 ? zy : nullptr, w_glo, P2, 1, out->yf, s))) return rc;
    if (out->sf && (rc = disco_apply(ctx, Xs, K > 1 ? zs : nullptr, w_glo, P2, 1, out->sf, s))) return rc;
    if (out->nf && (rc = disco_apply(ctx, Xn, K > 1 ? zn_ : nullptr, w_glo, P2, 1, out->nf, s))) return rc;
    return 0;
}
// ---- iterated (DANSE-style) continuation -------------------------------------------------------------------------------

static void iterated_steps(disco_ctx* ctx, const PathArgs& a, int iters, Steps& st) {
    const disco_cfg& c = ctx->cfg;
    const float *y = a.y, *mask_z = a.mask_z, *mask_w = a.mask_w;
    float* out = a.out;
    const PathBufs b = path_bufs(ctx, a);
    disco_c32 *X = b.X, *z = b.z, *yo = b.yo, *w_loc = b.w, *w_glo = b.w2;
    const int64_t G = (int64_t)c.rooms * c.nodes;
    const int M = c.mics, P2 = c.mics + c.nodes - 1;
    const bool same_mask = mask_w == mask_z;
    st.push_back({nullptr, false, [=](disco_stream s) { return stft_cov_partials(ctx, y, mask_z, X, s); }});
    st.push_back({"solve1", true, [=](disco_stream s) { return disco_gevd_mwf_r1_pending(ctx, c.mu, w_loc, nullptr, s); }});
    for (int it = 0; it < iters; ++it) {
        // compression with the current w_loc (step 1's, then the local part of the previous iteration's filter) and the step-2
        // statistics; only the last pass's z is read again (by the filter pass; it is what z_y returns)
        const bool last = it + 1 == iters;
        push_staged_step2(ctx, st, X, mask_w, same_mask, w_loc, z, last);
        st.push_back({"solve2", true, [=](disco_stream s) {
            int rc = disco_gevd_mwf_r1_pending(ctx, c.mu, w_glo, nullptr, s);
            if (rc || last) return rc;
            // yf of this iteration is not needed; the next one re-compresses with the local part of this iteration's filter
            const long long nb = (long long)G * ctx->F;
            hipLaunchKernelGGL(k_filter_head, dim3((unsigned)std::min<long long>((nb * M + 255) / 256, 65535)), dim3(256), 0, (hipStream_t)s,
                               (const c32*)w_glo, (c32*)w_loc, nb, M, P2);
            return check_launch(ctx, "k_filter_head");
        }});
    }
    push_apply2_istft(ctx, st, X, z, w_glo, a.yf, yo, out);
}

extern "C" int disco_tango_enhance_iterated(disco_ctx* ctx, const float* y, const float* mask_z, const float* mask_w, int iters,
                                            float* out, disco_c32* z_y, disco_c32* yf, void* workspace, size_t workspace_bytes,
                                            disco_stream s) {
    DISCO_ENTER(ctx);
    if (!y || !mask_z || !mask_w || !out || iters < 1) return fail(ctx, DISCO_E_ARG, "disco_tango_enhance_iterated: bad argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_enhance_iterated: node shard active");
    const WsLayout l = ws_layout(ctx);
    char* ws = nullptr;
    int rc = acquire_ws(ctx, workspace, workspace_bytes, l, &ws, "disco_tango_enhance_iterated");
    if (rc) return rc;
    const PathArgs a{y, mask_z, mask_w, out, z_y, yf, ws};
    // The overlapped form on the wide shapes: with the LDS group solver it lost (C5: 46.4 ms plain, 48.0 / 48.4 ms overlapped -- the room
    // pass takes a whole CU per workgroup and the solver's LDS blocks compete with it); with the register / DPP solver (k_solve_dpp.h:
    // 15 KB of LDS per wave, float64 VALU only) it pays: 38.40 -> 37.88 ms (profiles/r03_o_C5_overlap*.json).  Default like the fused route.
    return run_path(ctx, a, true, [iters](disco_ctx* x, const PathArgs& b, Steps& st) { iterated_steps(x, b, iters, st); }, s);
}
