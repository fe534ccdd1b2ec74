// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): the online / adaptive mode with COMPANIONS --
// the target and the noise image carried through the same per-frame filters as the mixture, which is what every score needs
// (tango.py:541-593).  The plain online entry points and their kernels live in api_online.hip; this unit holds the companion forms (csrc/k_online_ref.h) only.
#include "online_host.h"
#include "k_online_ref.h"
#include "k_stft.h"

using namespace disco;
using namespace disco_host;

// the walk with companions; `who` names the entry point in refusals.  Nothing is launched, and so nothing written, on a refusal.
static int online_mwf_ref_walk(disco_ctx* ctx, const char* who, const disco_c32* X, const disco_c32* Z, const float* mask, int P, float lambda_cor,
                               float mu, int update_every, float init_diag, disco_c32* out, disco_c32* w_last, const disco_online_companion* comp,
                               int n_comp, disco_stream s) {
    const disco_cfg& c = ctx->cfg;
    const OnlineWalk wk{ctx->T, ctx->T, 0, ctx->T, nullptr, 0, 0};
    OnlineArgs a;
    if (int rc = online_args(ctx, who, X, Z, mask, P, lambda_cor, mu, update_every, init_diag, out, w_last, wk, &a)) return rc;
    auto refuse = [&](const char* why) { return fail(ctx, DISCO_E_ARG, (std::string(who) + why).c_str()); };
    if (!comp || n_comp < 1 || n_comp > 2) return refuse(": one or two companions");
    OnlineComp cm{};
    cm.n = n_comp;
    for (int q = 0; q < n_comp; ++q) {
        if (!comp[q].X || !comp[q].out) return refuse(": a companion needs X and out");
        if (P > c.mics && !comp[q].Z) return refuse(": P > mics needs the exchanged z of every companion");
        cm.X[q] = (const c32*)comp[q].X;
        cm.Z[q] = P > c.mics ? (const c32*)comp[q].Z : nullptr;
        cm.out[q] = (c32*)comp[q].out;
    }
    hipStream_t st = (hipStream_t)s;
    // the routes of disco_online_mwf (api_online.hip), each in its companion form
    if (P <= 4 || (P <= 7 && ctx->opt[DISCO_OPT_SOLVE_THREAD] != 0)) {
        for_int<1, 7>(P, [&](auto p) { with_bool(P > 1 && ctx->opt[DISCO_OPT_ONLINE_SQ32] != 0, [&](auto sq32) {
            constexpr int P_ = decltype(p)::value, THREADS = solve_small_threads<P_>();
            constexpr bool SQ32 = P_ > 1 && decltype(sq32)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_online_mwf_thread_ref<P_, SQ32>), dim3((unsigned)((a.n_prob + THREADS - 1) / THREADS)),
                               dim3(THREADS), 0, st, a, cm);
        }); });
        return check_launch(ctx, "k_online_mwf_thread_ref");
    }
    const bool found = for_int<5, 16>(P, [&](auto p) {
        constexpr int P_ = decltype(p)::value;
        using Geom = SolveGeom<P_>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_online_mwf_ref<P_>), dim3((unsigned)((a.n_prob + Geom::PROBS - 1) / Geom::PROBS)), dim3(Geom::THREADS), 0,
                           st, a, cm);
    });
    if (!found) return refuse(": no kernel for this P");
    return check_launch(ctx, "k_online_mwf_ref");
}

extern "C" int disco_online_mwf_ref(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const float* mask, int P, float lambda_cor, float mu,
                                    int update_every, float init_diag, disco_c32* out, disco_c32* w_last, const disco_online_companion* comp,
                                    int n_comp, disco_stream s) {
    DISCO_ENTER(ctx);
    DISCO_REFUSE_LENGTHS(ctx, "disco_online_mwf_ref");
    return online_mwf_ref_walk(ctx, "disco_online_mwf_ref", X, Z, mask, P, lambda_cor, mu, update_every, init_diag, out, w_last, comp, n_comp, s);
}

// ---- the two-step online path with all nine reference outputs -----------------------------------------------------------------------
// The workspace is that of disco_tango_reference (ref_layout: three transforms, the three exchanged rows, the masks), whose three spare
// planes take yf, sf, nf when the caller wants only their time signals: disco_reserve(ctx, 2) covers both calls.
extern "C" size_t disco_online_reference_workspace_bytes(const disco_ctx* ctx) { return ctx ? ref_layout(ctx).total : 0; }

extern "C" int disco_tango_online_reference(disco_ctx* ctx, const float* y, const float* s_img, const float* n_img, const float* mask_z_in,
                                            const float* mask_w_in, float lambda_cor, int update_every, float init_diag,
                                            const disco_ref_outputs* out, float* time_out, void* workspace, size_t workspace_bytes,
                                            disco_stream s) {
    static const char* who = "disco_tango_online_reference";
    DISCO_ENTER(ctx);
    DISCO_REFUSE_LENGTHS(ctx, "disco_tango_online_reference");
    if (!y || !s_img || !n_img || !out) return fail(ctx, DISCO_E_ARG, "disco_tango_online_reference: null argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_online_reference: node shard active, drive disco_online_mwf_ref around an all-gather of z");
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics, K = c.nodes, P2 = M + K - 1;
    if (P2 > 16) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_online_reference: P = mics + nodes - 1 must be <= 16");
    if (c.mask_type < DISCO_MASK_IRM || c.mask_type > DISCO_MASK_IAM) return fail(ctx, DISCO_E_ARG, "disco_tango_online_reference: unknown mask type");
    if (!(lambda_cor >= 0.f && lambda_cor < 1.f) || update_every < 1 || !(init_diag > 0.f))
        return fail(ctx, DISCO_E_ARG, "disco_tango_online_reference: need 0 <= lambda < 1, update_every >= 1, init_diag > 0");
    const RefLayout l = ref_layout(ctx);
    char* ws = nullptr;
    if (int rcw = locate_ws(ctx, workspace, workspace_bytes, l.total, &ws, who)) return rcw;
    if (ctx->ref_ws == ws) ctx->ref_ws = nullptr;         // a steps = 1 state of disco_tango_reference in this workspace is overwritten
    hipStream_t st = (hipStream_t)s;
    const int64_t G = (int64_t)c.rooms * K;
    const long long nTF = (long long)G * ctx->T * ctx->F;
    const size_t plane_b = (size_t)nTF * sizeof(c32), mask_b = (size_t)nTF * sizeof(float);
    auto plane = [&](disco_c32* given, size_t off) { return given ? given : (disco_c32*)(ws + off); };
    disco_c32 *Xy = (disco_c32*)(ws + l.Xy), *Xs = (disco_c32*)(ws + l.Xs), *Xn = (disco_c32*)(ws + l.Xn);
    // every spectrum goes straight to the caller's array where one is given
    disco_c32 *zy = plane(out->z_y, l.zy), *zs = plane(out->z_s, l.zs), *zn_ = plane(out->z_n, l.zn_);
    disco_c32 *yf = plane(out->yf, l.znres), *sf = plane(out->sf, l.rows_s), *nf = plane(out->nf, l.rows_n);
    const float thr = powf(10.f, c.mask_bin_thr_db / 10.f);
    int rc;
    // ---- transforms of the mixture and of both images (tango.py:335-337)
    auto transforms = [&]() {
        int r = disco_stft(ctx, y, G, M, Xy, s);
        if (!r) r = disco_stft(ctx, s_img, G, M, Xs, s);
        if (!r) r = disco_stft(ctx, n_img, G, M, Xn, s);
        return r;
    };
    if ((rc = STAGE(ctx, s, "stft", transforms()))) return rc;
    // ---- the masks: the caller's, or the oracle TF mask at the reference microphone (step 1) and at channel 0 (step 2), as disco_tango_reference
    const float *mz = mask_z_in, *mw = mask_w_in;
    auto masks = [&]() {
        for (int step = 0; step < 2; ++step) {
            const float*& m = step ? mw : mz;
            float* wanted = step ? out->mask_w : out->masks_z;
            float* own = wanted ? wanted : (float*)(ws + (step ? l.mw : l.mz));      // computed straight into the caller's array where one is given
            if (!m) {
                ew_launch(k_tf_mask_channel, nTF, st, (const c32*)Xs, (const c32*)Xn, own, nTF, M, step ? 0 : c.ref_mic, c.mask_type, c.mask_pow, thr,
                          (const int*)nullptr, ctx->T, ctx->F, K);
                if (int r = check_launch(ctx, "k_tf_mask_channel")) return r;
                m = own;
            }
            if (wanted && wanted != m) HIPCHK(ctx, hipMemcpyAsync(wanted, m, mask_b, hipMemcpyDeviceToDevice, st));
        }
        return 0;
    };
    if ((rc = STAGE(ctx, s, "masks", masks()))) return rc;
    // ---- step 1 with companions: z_y, z_s, z_n (exchanged as complex64), then zn = Y[ref] - z_y (tango.py:376)
    const float mu = c.mu;
    const disco_online_companion c1[2] = {{Xs, nullptr, zs}, {Xn, nullptr, zn_}};
    if ((rc = STAGE(ctx, s, "online1_ref", online_mwf_ref_walk(ctx, who, Xy, nullptr, mz, M, lambda_cor, mu, update_every, init_diag, zy, nullptr, c1, 2, s))))
        return rc;
    if (out->zn && (rc = disco_noise_residual(ctx, Xy, zy, out->zn, s))) return rc;
    const disco_c32 *ys = zy, *ss = zs, *ns = zn_;          // the spectra whose inverse transforms time_out[0..2] are
    if (K == 1 && mw == mz) {                               // nothing to append: step 2 would repeat step 1
        const disco_c32* from[3] = {zy, zs, zn_};
        disco_c32* to[3] = {out->yf, out->sf, out->nf};
        for (int i = 0; i < 3; ++i)
            if (to[i]) HIPCHK(ctx, hipMemcpyAsync(to[i], from[i], plane_b, hipMemcpyDeviceToDevice, st));
    } else {
        // ---- step 2 on [Y_k ; z_y,j] with companions [S_k ; z_s,j] and [N_k ; z_n,j]: yf, sf, nf
        const disco_online_companion c2[2] = {{Xs, zs, sf}, {Xn, zn_, nf}};
        if ((rc = STAGE(ctx, s, "online2_ref",
                        online_mwf_ref_walk(ctx, who, Xy, zy, mw, P2, lambda_cor, mu, update_every, init_diag, yf, nullptr, c2, 2, s))))
            return rc;
        ys = yf, ss = sf, ns = nf;
    }
    if (!time_out) return 0;
    // ---- the six signals of the scores, in the order yf, sf, nf, z_y, z_s, z_n (one frame per transform, as disco_tango_online)
    const size_t sig = (size_t)G * c.length;
    auto inverse = [&]() {
        const disco_c32* spec[6] = {ys, ss, ns, zy, zs, zn_};
        for (int i = 0; i < 6; ++i)
            if (int r = istft_any(ctx, spec[i], G, time_out + i * sig, c.length, ctx->T, s, true)) return r;
        return 0;
    };
    return STAGE(ctx, s, "istft", inverse());
}
