// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): online / adaptive mode
#include "online_host.h"

using namespace disco;
using namespace disco_host;

// ---- online / adaptive mode ------------------------------------------------------------------------------

namespace disco_host {
int online_args(disco_ctx* ctx, const char* who, const disco_c32* X, const disco_c32* Z, const float* mask, int P, float lambda_cor, float mu,
                int update_every, float init_diag, disco_c32* out, disco_c32* w_last, const OnlineWalk& wk, OnlineArgs* args) {
    const disco_cfg& c = ctx->cfg;
    auto refuse = [&](int code, const char* why) { return fail(ctx, code, (std::string(who) + why).c_str()); };
    if (!X || !mask || !out) return refuse(DISCO_E_ARG, ": null argument");
    if (P != c.mics && P != c.mics + c.nodes - 1) return refuse(DISCO_E_ARG, ": P must be mics or mics + nodes - 1");
    if (P > c.mics && !Z) return refuse(DISCO_E_ARG, ": P > mics needs the exchanged z");
    if (!(lambda_cor >= 0.f && lambda_cor < 1.f) || update_every < 1 || !(init_diag > 0.f))
        return refuse(DISCO_E_ARG, ": need 0 <= lambda < 1, update_every >= 1, init_diag > 0");
    if (P > 16) return refuse(DISCO_E_UNSUPPORTED, ": P must be <= 16");
    OnlineArgs& a = *args;
    a.X = (const c32*)X;
    a.Z = P > c.mics ? (const c32*)Z : nullptr;
    a.mask = mask;
    a.out = (c32*)out;
    a.w_last = (c32*)w_last;
    a.K = c.nodes;
    a.Kl = ctx->Kl;
    a.k0 = ctx->k0;
    a.T = wk.T;
    a.Tx = wk.Tx;
    a.tx0 = wk.tx0;
    a.Tm = wk.Tm;
    a.state = wk.state;
    a.init = wk.init;
    a.phase = wk.phase;
    a.F = ctx->F;
    a.M = c.mics;
    a.update_every = update_every;
    a.lambda_cor = lambda_cor;
    a.init_diag = init_diag;
    a.mu = (double)mu;
    a.n_prob = (long long)c.rooms * ctx->Kl * ctx->F;
    a.zblk = ctx->zblk;
    a.R = c.rooms;
    return 0;
}
}  // namespace disco_host

static int online_mwf_walk(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const float* mask, int P, float lambda_cor, float mu,
                           int update_every, float init_diag, disco_c32* out, disco_c32* w_last, const OnlineWalk& wk, disco_stream s) {
    OnlineArgs a;
    if (int rc = online_args(ctx, "disco_online_mwf", X, Z, mask, P, lambda_cor, mu, update_every, init_diag, out, w_last, wk, &a)) return rc;
    hipStream_t st = (hipStream_t)s;
    // P <= 4, and 5 <= P <= 7 under option "solve_thread": one thread per (room, node, bin) (the float64 solve in the registers of one thread,
    // AGPRs as its second register file: k_solve_small.h)
    if (P <= 4 || (P <= 7 && ctx->opt[DISCO_OPT_SOLVE_THREAD] != 0)) {
        for_int<1, 7>(P, [&](auto p) { with_bool(P > 1 && ctx->opt[DISCO_OPT_ONLINE_SQ32] != 0, [&](auto sq32) {      // the squarings in packed float32
            constexpr int P_ = decltype(p)::value, THREADS = solve_small_threads<P_>();
            constexpr bool SQ32 = P_ > 1 && decltype(sq32)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_online_mwf_thread<P_, SQ32>), dim3((unsigned)((a.n_prob + THREADS - 1) / THREADS)),
                               dim3(THREADS), 0, st, a);
        }); });
        return check_launch(ctx, "k_online_mwf_thread");
    }
    const bool found = for_int<5, 16>(P, [&](auto p) {         // a group of 8 / 16 lanes per (room, node, bin)
        constexpr int P_ = decltype(p)::value;
        using Geom = SolveGeom<P_>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_online_mwf<P_>), dim3((unsigned)((a.n_prob + Geom::PROBS - 1) / Geom::PROBS)), dim3(Geom::THREADS), 0,
                           st, a);
    });
    if (!found) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_online_mwf: no kernel for this P");
    return check_launch(ctx, "k_online_mwf");
}

extern "C" int disco_online_mwf(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const float* mask, int P,
                                float lambda_cor, float mu, int update_every, float init_diag, disco_c32* out,
                                disco_c32* w_last, disco_stream s) {
    DISCO_ENTER(ctx);
    DISCO_REFUSE_LENGTHS(ctx, "disco_online_mwf");
    const OnlineWalk wk{ctx->T, ctx->T, 0, ctx->T, nullptr, 0, 0};
    return online_mwf_walk(ctx, X, Z, mask, P, lambda_cor, mu, update_every, init_diag, out, w_last, wk, s);
}

extern "C" int disco_tango_online(disco_ctx* ctx, const float* y, const float* mask_z, const float* mask_w, float lambda_cor,
                                  int update_every, float init_diag, float* out, disco_c32* z_y, disco_c32* yf,
                                  void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    DISCO_REFUSE_LENGTHS(ctx, "disco_tango_online");
    if (!y || !mask_z || !mask_w || !out) return fail(ctx, DISCO_E_ARG, "disco_tango_online: null argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_online: node shard active, drive disco_online_mwf around an all-gather of z");
    const disco_cfg& c = ctx->cfg;
    const WsLayout l = ws_layout(ctx);
    char* ws = nullptr;
    int rc = acquire_ws(ctx, workspace, workspace_bytes, l, &ws, "disco_tango_online");
    if (rc) return rc;
    disco_c32* X = (disco_c32*)(ws + l.X);
    disco_c32* z = z_y ? z_y : (disco_c32*)(ws + l.z);
    disco_c32* yo = yf ? yf : (disco_c32*)(ws + l.yf);
    const int64_t G = (int64_t)c.rooms * c.nodes;
    if ((rc = STAGE(ctx, s, "stft", disco_stft(ctx, y, G, c.mics, X, s)))) return rc;
    if ((rc = STAGE(ctx, s, "online1", disco_online_mwf(ctx, X, nullptr, mask_z, c.mics, lambda_cor, c.mu, update_every, init_diag, z, nullptr, s)))) return rc;
    if (c.nodes == 1 && mask_w == mask_z) {             // nothing to append: step 2 would repeat step 1
        if (yf) HIPCHK(ctx, hipMemcpyAsync(yf, z, (size_t)G * ctx->T * ctx->F * sizeof(c32), hipMemcpyDeviceToDevice, (hipStream_t)s));
        return istft_any(ctx, z, G, out, c.length, ctx->T, s, true);
    }
    if ((rc = STAGE(ctx, s, "online2", disco_online_mwf(ctx, X, z, mask_w, c.mics + c.nodes - 1, lambda_cor, c.mu, update_every, init_diag, yo, nullptr, s)))) return rc;
    return STAGE(ctx, s, "istft", istft_any(ctx, yo, G, out, c.length, ctx->T, s, true));       // one frame per transform: see k_istft
}

// ---- the online path as a STREAM: state in, state out (SURVEY 8f-2 "streaming latency instead of batch") -----------------------------
// One call consumes n_hops hops of new samples per channel and emits every output sample that became final.  Frame t (centred at
// sample t * hop) needs the samples up to t * hop + n_fft / 2, so after h hops of input the frames 0 ... h - 1 exist and the output samples
// [0, (h - 1) hop) are final (a sample takes its two overlapping frames): the latency is one hop plus the chunk.  `last` adds the frame
// centred at the end of the signal (its second half is the padding of the whole-clip transform) and flushes the rest.
// What a call keeps for the next one lives in the CALLER'S state block: the last hop of samples of every channel (the first half of the
// next frame), the last output spectrum (the first half of the next overlap-add), both smoothed matrices and the filter in force of every
// (room, node, bin) of both steps.  The arithmetic per frame is that of disco_tango_online -- same kernels on a transform block of the
// chunk's frames -- so N chunks reproduce one whole-clip call BIT FOR BIT (tests: check_online_stream).
namespace {
struct StreamLayout {
    size_t tail, yf_last, st1, st2, total;
};
StreamLayout stream_layout(const disco_ctx* ctx) {
    const disco_cfg& c = ctx->cfg;
    const size_t G = (size_t)c.rooms * c.nodes, F = ctx->F, M = c.mics, P2 = c.mics + c.nodes - 1;
    StreamLayout l;
    size_t o = 0;
    l.tail = o;
    o += align_up(G * M * c.hop * sizeof(float));
    l.yf_last = o;
    o += align_up(G * F * sizeof(c32));
    l.st1 = o;
    o += align_up(G * F * (M * (M + 1) + M) * sizeof(c32));                 // lower triangles of both smoothed matrices + the filter (k_online.h)
    l.st2 = o;
    o += align_up(G * F * (P2 * (P2 + 1) + P2) * sizeof(c32));
    l.total = o;
    return l;
}
struct StreamWs {
    size_t y, X, z, y2, total;
};
StreamWs stream_ws(const disco_ctx* ctx, int n_hops) {
    const disco_cfg& c = ctx->cfg;
    const size_t G = (size_t)c.rooms * c.nodes, F = ctx->F, M = c.mics, n = (size_t)n_hops;
    StreamWs w;
    size_t o = 0;
    w.y = o;
    o += align_up(G * M * (n + 1) * c.hop * sizeof(float));              // [last hop kept | new samples] per channel
    w.X = o;
    o += align_up(G * (n + 2) * F * M * sizeof(c32));                    // its transform block; afterwards [last spectrum kept | new spectra] per signal
    w.z = o;
    o += align_up(G * (n + 1) * F * sizeof(c32));                        // step 1's output of the call's frames
    w.y2 = o;
    o += align_up(G * (n + 1) * F * sizeof(c32));                        // step 2's
    w.total = o;
    return w;
}
}  // namespace

extern "C" size_t disco_online_state_bytes(const disco_ctx* ctx) { return ctx ? stream_layout(ctx).total : 0; }
extern "C" size_t disco_online_stream_workspace_bytes(const disco_ctx* ctx, int max_hops) {
    return (ctx && max_hops > 0) ? stream_ws(ctx, max_hops).total : 0;
}

extern "C" int disco_tango_online_stream(disco_ctx* ctx, const float* y_new, int n_hops, const float* mask_z, const float* mask_w,
                                         float lambda_cor, int update_every, float init_diag, int64_t hops_before, int last, void* state,
                                         float* out, void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    DISCO_REFUSE_LENGTHS(ctx, "disco_tango_online_stream");
    const disco_cfg& c = ctx->cfg;
    if (!y_new || !mask_z || !mask_w || !out || !state || !workspace) return fail(ctx, DISCO_E_ARG, "disco_tango_online_stream: null argument");
    if (n_hops < 1 || hops_before < 0 || update_every < 1)
        return fail(ctx, DISCO_E_ARG, "disco_tango_online_stream: need n_hops >= 1, hops_before >= 0, update_every >= 1");
    if (hops_before == 0 && n_hops < 2)
        return fail(ctx, DISCO_E_ARG, "disco_tango_online_stream: the first call needs two hops (the transform's padding reflects the first half window)");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_online_stream: node shard active");
    const StreamWs w = stream_ws(ctx, n_hops);
    if (workspace_bytes < w.total)
        return fail(ctx, DISCO_E_ARG, "disco_tango_online_stream: workspace smaller than disco_online_stream_workspace_bytes(ctx, n_hops)");
    const StreamLayout l = stream_layout(ctx);
    const bool first = hops_before == 0;
    const int H = c.hop, F = ctx->F, M = c.mics, P2 = c.mics + c.nodes - 1;
    const int64_t G = (int64_t)c.rooms * c.nodes;
    const int n_new = n_hops + (last ? 1 : 0);                       // frames this call completes: hops_before ... hops_before + n_new - 1
    char* st = (char*)state;
    char* ws = (char*)workspace;
    float* tail = (float*)(st + l.tail);
    c32* yf_last = (c32*)(st + l.yf_last);
    float* ym = (float*)(ws + w.y);
    disco_c32* X = (disco_c32*)(ws + w.X);
    disco_c32* z = (disco_c32*)(ws + w.z);
    hipStream_t hs = (hipStream_t)s;
    // ---- the transform block: [kept hop | new samples] per channel (first call: the new samples alone -- the transform pads its start)
    const int Lm = (first ? 0 : H) + n_hops * H;
    const size_t rows = (size_t)G * M;
    // [kept hop | new samples] per channel, and the last new hop becomes the kept one (the next call's first half window): one launch
    hipLaunchKernelGGL(k_stream_shift, dim3((unsigned)std::min<size_t>((rows * H + 255) / 256, 1 << 16)), dim3(256), 0, hs, tail, y_new, ym, (long long)rows, H,
                       n_hops, first ? 0 : 1);
    if (int rcl = check_launch(ctx, "k_stream_shift")) return rcl;
    const int Tb = 1 + Lm / H;                                       // frames of the block; this call's: [first ? 0 : 1, + n_new)
    int rc = stft_any(ctx, ym, G, M, X, Lm, Tb, s);
    if (rc) return rc;
    // ---- the two recursions, resumed from the caller's state (a filter update falls on the frames that are multiples of update_every)
    const int phase = (int)((update_every - hops_before % update_every) % update_every);
    OnlineWalk wk{n_new, Tb, first ? 0 : 1, n_new, (c32*)(st + l.st1), first ? 1 : 0, phase};
    if ((rc = online_mwf_walk(ctx, X, nullptr, mask_z, M, lambda_cor, c.mu, update_every, init_diag, z, nullptr, wk, s))) return rc;
    const c32* ynew = (const c32*)z;                                 // [G][n_new][F]: what is overlap-added
    if (!(c.nodes == 1 && mask_w == mask_z)) {                       // (a single node under one mask: step 2 would repeat step 1)
        disco_c32* y2 = (disco_c32*)(ws + w.y2);
        wk.state = (c32*)(st + l.st2);
        if ((rc = online_mwf_walk(ctx, X, z, mask_w, P2, lambda_cor, c.mu, update_every, init_diag, y2, nullptr, wk, s))) return rc;
        ynew = (const c32*)y2;
    }
    // ---- overlap-add over [kept spectrum | new spectra] per signal: the samples between consecutive frame centres are final
    const int Ty = n_new + (first ? 0 : 1);
    c32* blk = (c32*)(ws + w.X);                                     // the transform block is dead now: the interleaved spectra go there
    // [kept spectrum | new spectra] per signal, and the last new spectrum becomes the kept one (the next call's first half of the overlap)
    hipLaunchKernelGGL(k_stream_shift, dim3((unsigned)std::min<size_t>(((size_t)G * 2 * F + 255) / 256, 1 << 16)), dim3(256), 0, hs, (float*)yf_last,
                       (const float*)ynew, (float*)blk, (long long)G, 2 * F, n_new, first ? 0 : 1);
    if (int rcl = check_launch(ctx, "k_stream_shift")) return rcl;
    if (Ty >= 2 && (rc = istft_any(ctx, (const disco_c32*)blk, G, out, (Ty - 1) * H, Ty, s, true))) return rc;
    return 0;
}
