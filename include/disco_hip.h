/*
 * disco_hip.h -- C ABI of libdisco_hip.so: the MI355X (gfx950) implementation of DISCO's
 * distributed multichannel-Wiener-filter speech-enhancement hot path.
 *
 * The reference (nfurnon/disco) is pure Python and has no FFI seam; its boundary for this path is the
 * Python call surface listed below.  Every entry point of this header replaces one of those functions
 * (or one loop nest inside `offline_tango`); the Python shim in disco_amd/ keeps the reference's names
 * and argument meaning on top of it.  The ctypes binding a reference maintainer would add is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers owned by the caller (except where "host" is stated).
 *   - complex64 is interleaved (re, im) float pairs  == numpy complex64 == disco_c32.
 *   - Every compute call is asynchronous on the given hipStream_t (pass NULL for the default stream);
 *     no hidden synchronisation.  A disco_ctx is bound to cfg.device and is not thread-safe: every entry point switches to
 *     that device for its own duration and restores the calling thread's current device before it returns.
 *   - Return value: 0 on success, DISCO_E_ARG (-1) bad argument, DISCO_E_UNSUPPORTED (-2) unsupported
 *     shape, -1000 - hipError_t for a HIP failure.  Never throws, never aborts.
 *     disco_last_error(ctx) returns a static/ctx-owned message for the last failing call.
 *
 * Layouts (frame-major; R rooms, K nodes/room, M mics/node, L samples, T = 1 + L/hop frames,
 * F = n_fft/2 + 1 bins, P = channels seen by a filter: M in step 1, M + K - 1 in step 2):
 *   time signals   float    [R][K][M][L]            (the reference's [node][channel] -> time, tango.py:259-261)
 *   STFT           disco_c32[R][K][T][F][M]         (mic innermost: one coalesced 8*M-byte vector per (t,f))
 *   masks          float    [R][K][T][F]
 *   z / filtered   disco_c32[R][K][T][F]
 *   covariances    disco_c32[R][K][F][P][P]         (row-major Hermitian, what intern_filter(Rxx, Rnn) takes per bin)
 *   filters w, t1  disco_c32[R][K][F][P]
 *   The Python-visible (F, T) arrays of the reference are transposes of the [T][F] planes.
 */
#ifndef DISCO_HIP_H
#define DISCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DISCO_E_ARG          (-1)
#define DISCO_E_UNSUPPORTED  (-2)
#define DISCO_E_HIP_BASE     (-1000)

#define DISCO_MASK_IRM 0
#define DISCO_MASK_IBM 1
#define DISCO_MASK_IAM 2

/* disco_cfg.flags: run step 2 of disco_tango_enhance through the staged kernels (z materialised in HBM, the form a
 * node-sharded multi-GPU run needs) instead of the default in-register exchange. */
#define DISCO_FLAG_STAGED_STEP2 1
/* disco_cfg.flags: do not size the covariance partial-sum blocks at disco_create; they are then allocated by the first call
 * that needs them (a hipMalloc inside that call).  For contexts that only ever run the transforms / masks / metrics. */
#define DISCO_FLAG_LAZY_SCRATCH 2
/* disco_cfg.flags: never create the half-batch children of the overlapped whole-path calls (option "overlap_solves"), whatever the
 * batch size: the context then owns one set of partial-sum blocks only. */
#define DISCO_FLAG_NO_CHILDREN 4

#define DISCO_PAD_REFLECT  0   /* librosa < 0.10 (the reference's era)  */
#define DISCO_PAD_CONSTANT 1   /* librosa >= 0.10                        */

typedef struct disco_c32 { float re, im; } disco_c32;
typedef struct disco_ctx disco_ctx;
typedef void* disco_stream;                 /* a hipStream_t */

/* Mirrors the module constants of tango.py:28-38 (N_FFT, N_HOP, nb_ch, ref_mics, SNR/mask choices)
 * plus the batch size.  All int/float, no pointers: safe to fill from any FFI. */
typedef struct disco_cfg {
    int32_t rooms;          /* R  independent rooms in the batch                                  */
    int32_t nodes;          /* K  nodes per room            (len(nb_ch), tango.py:31)              */
    int32_t mics;           /* M  microphones per node      (nb_ch[k], uniform)                    */
    int32_t length;         /* L  samples per channel                                               */
    int32_t n_fft;          /* N_FFT, 512 or 1024           (tango.py:28)                           */
    int32_t hop;            /* N_HOP, must be n_fft/2       (tango.py:29)                           */
    int32_t ref_mic;        /* ref_mics[k]                  (tango.py:32)                           */
    int32_t mask_type;      /* DISCO_MASK_*  ('irmX'/'ibmX'/'iamX', dnn/utils.py:57-67)             */
    int32_t mask_pow;       /* X of 'irmX'                                                          */
    float   mask_bin_thr_db;/* bin_thr of tf_mask                                                   */
    float   mu;             /* speech-distortion constant of intern_filter (1 at every call site)   */
    int32_t pad_mode;       /* DISCO_PAD_*                                                          */
    int32_t device;         /* HIP device ordinal                                                   */
    int32_t flags;          /* DISCO_FLAG_*                                                         */
    int32_t reserved[2];
} disco_cfg;

/* ---- lifetime ------------------------------------------------------------------------------------ */
const char* disco_version(void);
int  disco_create(disco_ctx** out, const disco_cfg* cfg);
void disco_destroy(disco_ctx* ctx);
const char* disco_last_error(const disco_ctx* ctx);      /* ctx may be NULL: last create() error       */
int  disco_n_frames(const disco_ctx* ctx);               /* T = 1 + L/hop   (librosa center=True)      */
int  disco_n_freq(const disco_ctx* ctx);                 /* F = n_fft/2 + 1                            */
/* Bytes of device workspace disco_tango_enhance needs for this cfg (STFT + z + yf + covariances). */
size_t disco_workspace_bytes(const disco_ctx* ctx);

/* Device memory the library owns.  disco_create sizes the two covariance partial-sum blocks for the cfg and the launch geometry
 * (unless DISCO_FLAG_LAZY_SCRATCH); disco_set_tuning re-sizes them.  disco_reserve(ctx, 1) additionally allocates the context's
 * own whole-path workspace (disco_workspace_bytes) that disco_tango_enhance / _iterated / _online fall back to when the caller
 * passes workspace = NULL; disco_reserve(ctx, 2) sizes it for disco_tango_reference as well (disco_reference_workspace_bytes);
 * disco_reserve(ctx, 0) only re-sizes the partial-sum blocks (e.g. after disco_set_node_shard).  After it, none of the whole-path or stage entry points allocates, frees or synchronises:
 * a call is a fixed sequence of kernel launches on the caller's stream and can be captured into a hipGraph
 * (hipStreamBeginCapture on that stream, stage timers off) and replayed.  (disco_rir_convolve keeps its own lazy workspace.) */
int  disco_reserve(disco_ctx* ctx, int own_workspace);
/* Bytes of device memory the context owns right now (partial-sum blocks + own workspace + convolution workspace): unchanged
 * across a call <=> that call allocated nothing. */
size_t disco_owned_bytes(const disco_ctx* ctx);

/* Node-sharded operation (SURVEY 8e "finer sharding"): this context holds only nodes [first_node, first_node + count)
 * of every room; the other nodes live on other GPUs and their compressed signals arrive through an all-gather of z
 * (RCCL) between step 1 and step 2 -- the one exchange DISCO's algorithm performs (tango.py:378-386).
 * Afterwards every per-node array of the STAGED entry points (X, masks, out/z of disco_apply, Rss/Rnn, w) has
 * `count` nodes per room, while Zs/Zn/Z keep all cfg.nodes nodes (global order).  The fused entry points and
 * disco_tango_enhance need all nodes on one GPU and return DISCO_E_UNSUPPORTED while a shard is active. */
int  disco_set_node_shard(disco_ctx* ctx, int first_node, int node_count);

/* Layout of the exchanged signals handed to the STAGED entry points (Zs / Zn of disco_cov_masked, Z of disco_apply and
 * disco_online_mwf).  Default: [R][K][T][F].  After an all-gather over W = K / nodes_per_block ranks the signals arrive rank-major,
 * [W][R][nodes_per_block][T][F]; disco_set_z_blocks(ctx, nodes_per_block) makes the kernels read that layout directly, so the
 * node-sharded driver needs no transposing copy between the collective and step 2.  nodes_per_block = cfg.nodes restores the
 * default.  Outputs (z written by disco_apply for the LOCAL nodes) keep [R][count][T][F]: that IS a rank's block. */
int  disco_set_z_blocks(disco_ctx* ctx, int nodes_per_block);

/* Per-room clip lengths: rooms of different durations in one batch.  The arrays keep their rectangular shapes ([R][K][M][cfg.length],
 * [R][K][T][F] with T = disco_n_frames, which does not change); room r is processed as if it had been run alone in a context of
 * length = lengths[r], with T_r = 1 + lengths[r] / hop frames:
 *   - samples at and beyond lengths[r] are never read (they may hold anything, NaN included): the transform reflects or zero-pads at
 *     lengths[r].  The metrics honour the same promise through a stop per signal: disco_pair_stats_spans, disco_band_stats_spans,
 *     disco_lag_corr_spans, disco_bss_eval_spans, disco_bss_estimates, disco_stoi and disco_estoi read nothing at or beyond a signal's stop;
 *   - frames t >= T_r do not exist: they enter no statistic; spectra, z, yf and the masks the library computes are exact zeros there.
 *     Masks the CALLER passes in must be FINITE in those frames (their values do not matter);
 *   - output samples n < lengths[r] are the inverse transform with the window sum of T_r frames, n >= lengths[r] exact zeros;
 *   - disco_cov_masked / disco_stft_cov_fused, when they return matrices, divide room r's sums by T_r.
 * lengths: HOST array of cfg.rooms int32 (copied; the context owns the device copy, allocated here and never inside a compute call),
 * or NULL to restore the uniform batch.  pad_mode reflect: n_fft/2 < lengths[r] <= cfg.length (the rule disco_create applies to
 * cfg.length); constant: 1 <= lengths[r] <= cfg.length.  Otherwise DISCO_E_ARG, state unchanged.  lengths[r] == cfg.length for every r
 * gives bit for bit the results of the uniform batch.  A second call rewrites the same device block in place (the kernels read the
 * lengths from device memory; launch geometry and workspace sizes do not depend on them), so a hipGraph captured with lengths set
 * replays with the lengths in force at replay.
 * Covered: disco_stft, disco_istft, disco_mask_oracle (signal g of n_sig belongs to room g / (n_sig / cfg.rooms); n_sig not a multiple
 * of cfg.rooms is DISCO_E_ARG while lengths are set), disco_cov_masked, disco_stft_cov_fused, disco_step2_*_fused,
 * disco_apply_istft_fused, and every route of disco_tango_enhance, disco_tango_enhance_iterated and disco_tango_reference.
 * Refused with DISCO_E_UNSUPPORTED while lengths are set: disco_online_mwf, disco_tango_online, disco_tango_online_stream,
 * disco_mask_ivad, a node shard (disco_set_node_shard; and disco_set_lengths while a shard is active).  disco_tf_mask is element-wise and
 * knows no frames: it computes every element it is given. */
int  disco_set_lengths(disco_ctx* ctx, const int32_t* lengths, int n_rooms);

/* Launch geometry.  By default every kernel derives its work split from the batch size (long per-wave frame runs and single
 * covariance chunks once R*K fills the chip, short runs and up to 8 chunks for small batches).  This call pins it, so that a
 * SMALL batch can be run -- and checked against the oracle -- on exactly the code path a large production batch takes:
 *   stft_frames_per_wave  frames each wave of disco_stft_cov_fused streams (a workgroup covers 4x that; heuristic 8..80)
 *   cov_chunks            frame chunks of disco_cov_masked                            (heuristic 1..8)
 *   step2_chunks          frame chunks of disco_step2_cov_fused / disco_step2_apply_fused (heuristic 1..8)
 *   istft_pairs           frame pairs per workgroup of disco_step2_apply_istft_fused  (heuristic 4..64)
 * 0 keeps the heuristic for that kernel.  Results do not depend on the geometry beyond float32 summation order. */
int  disco_set_tuning(disco_ctx* ctx, int stft_frames_per_wave, int cov_chunks, int step2_chunks, int istft_pairs);

/* Per-context options: integer switches that choose between equivalent kernel routes (A/B measurements, tests of both routes).
 * Two contexts of one process may differ; nothing is read from the environment inside a compute call -- an environment variable
 * (named below) only PRESETS the option when disco_create runs.  The route a whole-path call took shows in the stage names of
 * disco_stage_report.  Keys:
 *   "room_cov"           (DISCO_ROOM_COV, default 1)   wide shapes (M + K - 1 > 8): z + step-2 statistics of a whole room in one persistent pass
 *                         ("room_cov2", csrc/k_room.h) instead of disco_apply + disco_cov_masked ("apply1" + "cov2": the staged route,
 *                         which a node shard takes in any case)
 *   "overlap_solves"     (DISCO_OVERLAP_SOLVES, 1)  disco_tango_enhance / _iterated on batches of rooms x nodes >= 1024 run as two
 *                         half-batches, the second on an internal stream forked from / joined to the caller's with events (still one
 *                         capturable launch sequence): one half's solves overlap the other half's streaming kernels.  Each stage
 *                         then shows 2 launches of R/2 rooms.  2: force it for any batch of >= 2 rooms (tests); 0: off.  The
 *                         half-batch contexts (own partial-sum blocks) are created by disco_create / disco_set_option
 *   "solve_thread"       (DISCO_SOLVE_THREAD, 1) rank-1 GEVD-MWF solves with 5 <= P <= 8 (and the online mode with 5 <= P <= 7) run one THREAD per
 *                         pencil (csrc/k_solve_small.h: Hermitian halves in registers, AGPRs as the second register file at P = 8): 0.26 against
 *                         0.61 ms per 1 028 000 P = 7 pencils, 0.39 against 0.81 at P = 8; 0: the LDS group solver (csrc/k_solve.h), the
 *                         cross-check route of the solver tests.  P <= 4 always runs per thread
 *   "solve_dpp"          (DISCO_SOLVE_DPP, 1)  rank-1 GEVD-MWF solves with 9 <= P <= 16 run in registers, other lanes' entries read through
 *                         DPP row broadcasts (csrc/k_solve_dpp.h: 3.7 instead of 7.2 ms per C5 launch); 0: the LDS group solver.  Same
 *                         algorithm and breakdown rules; the two are tested against each other (check_solver_routes)
 *   "online_sq32"        (DISCO_ONLINE_SQ32, 1) online mode, thread solves (P <= 7): the repeated squarings on packed float32 (v_pk_fma_f32), Cholesky,
 *                         whitening, back substitution and the Rayleigh quotient in float64 (csrc/k_solve_small.h): 193 instead of 240 ms per
 *                         C3-shaped 1000-room step (52x instead of 42x real-time), the same 2.0e-6 from the oracle; 0: float64 squarings.  The
 *                         offline solves always square in float64
 *   "fuse_wide_istft"    (DISCO_FUSE_WIDE_ISTFT, 1) disco_tango_enhance / _iterated on the wide shapes (M + K - 1 > 8; 512 / 1024-point STFT) end in ONE
 *                         filter + iSTFT pass (csrc/k_fused.h k_apply_istft_wide, stage "apply2_istft": the filtered spectra stay on chip, and are
 *                         written only when the caller asks for yf) instead of disco_apply + disco_istft ("apply2" + "istft": what the ABI's
 *                         stage calls and a node shard run)
 *   "packed_x"           (DISCO_PACKED_X, 1) disco_tango_enhance on the on-chip-exchange route when yf is not asked for (nodes >= 2, M + K - 1 <= 8,
 *                         512-point STFT: stages "stft_cov1", "step2_cov", "step2_apply_istft") keeps the spectra, which then never leave the
 *                         workspace, in rows of F - 1 bins -- [R][K][T][F - 1][M], slot 0 of a channel = (Re X[0], Re X[F - 1]): DC and Nyquist of
 *                         a real frame are real.  A row is then a whole number of 128-byte lines (the public row of 8 M F bytes is not), so no
 *                         wave load or store of the three passes straddles one.  Same results (np.array_equal); the workspace size does not
 *                         depend on the option; 0: the public layout [T][F][M] there too.  Every argument X of the ABI is [T][F][M] in any case
 * Routes that earlier rounds measured slower or less accurate and kept "as a record" are gone from the library (round 5): the filter +
 * iSTFT pass from the samples, the register-staged room pass, the mixed-precision group solver, 4 time sub-chunks in the room pass, the
 * float32 step-1 statistics of the wide shapes, the solves-only side stream.  Their measurements are in profiles/.
 * Unknown key: DISCO_E_ARG. */
int  disco_set_option(disco_ctx* ctx, const char* key, int value);
int  disco_get_option(const disco_ctx* ctx, const char* key, int* value);

/* Per-stage timers of the whole-path entry points (disco_tango_enhance, _iterated, _online) and of disco_mask_oracle:
 * while enabled, every stage they launch (STFT+covariance, solves, filter passes, iSTFT ...) is bracketed by two hipEvents on
 * the call's stream.  disco_stage_timing(ctx, 1) clears and starts, (ctx, 0) clears and stops.  disco_stage_report waits for
 * the recorded events and returns the number of distinct stages n <= max_stages, with names[i*32 .. i*32+31] (NUL-terminated),
 * total_ms[i] (sum over the recorded launches), launches[i] and rooms[i] (rooms processed, summed over the launches: a stage of the
 * iterated scheme runs twice over the whole batch, a stage of an overlapped call once over each half; may be NULL); all HOST arrays.
 * Nothing is timed, recorded or synchronised while disabled (the default). */
int  disco_stage_timing(disco_ctx* ctx, int enable);
int  disco_stage_report(disco_ctx* ctx, char* names, float* total_ms, int* launches, int64_t* rooms, int max_stages);

/* ---- plain device-memory helpers (so a numpy-only host can drive the library without torch) -------- */
int  disco_dev_alloc(disco_ctx* ctx, size_t bytes, void** dptr);
int  disco_dev_free(disco_ctx* ctx, void* dptr);
int  disco_h2d(disco_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, disco_stream s);
int  disco_d2h(disco_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, disco_stream s);
int  disco_sync(disco_ctx* ctx, disco_stream s);         /* hipStreamSynchronize                        */

/* ---- stage kernels --------------------------------------------------------------------------------- */

/* librosa.core.stft(x, n_fft, hop, center=True)  -- tango.py:335-337, math_utils.py:134-140 (my_stft).
 * x: float [n_sig][chans][L]  ->  X: disco_c32 [n_sig][T][F][chans].  n_sig = R*K and chans = M on the hot path. */
int disco_stft(disco_ctx* ctx, const float* x, int64_t n_sig, int chans, disco_c32* X, disco_stream s);

/* librosa.core.istft(Z, hop, win_length=n_fft, center=True, length=L) -- tango.py:528-539, math_utils.py:143-152.
 * Z: disco_c32 [n_sig][T][F]  ->  out: float [n_sig][L]. */
int disco_istft(disco_ctx* ctx, const disco_c32* Z, int64_t n_sig, float* out, disco_stream s);

/* tf_mask(s, n, type, bin_thr) on STFT planes -- dnn/utils.py:44-71.  Elementwise over n_elem bins. */
int disco_tf_mask(disco_ctx* ctx, const disco_c32* S, const disco_c32* N, int64_t n_elem,
                  int mask_type, int mask_pow, float bin_thr_db, float* mask, disco_stream s);

/* Oracle mask straight from time signals (get_mask -> tf_mask at the reference mic, tango.py:338-342):
 * s_ref, n_ref: float [n_sig][L] (target / noise image at the reference mic) -> mask float [n_sig][T][F].
 * Fuses the two STFTs (one complex FFT for the pair) with the mask; uses cfg.mask_type / mask_pow. */
int disco_mask_oracle(disco_ctx* ctx, const float* s_ref, const float* n_ref, int64_t n_sig,
                      float* mask, disco_stream s);

/* The masks of a meeting room of n_src simultaneous talkers and the spectrum of their mix, in one transform pass (get_masks,
 * dataset_generation/gen_meetit/convolve_signals.py:166-188).  images: float [n_src][n_sig][L], source-major (n_sig = rooms * channels)
 * -> masks float [n_src][n_sig][T][F] and, unless NULL, mix disco_c32 [n_sig][T][F].  With X_j the STFT of images[j]:
 *   mix     = ((X_0 + X_1) + X_2) + ...            complex64 sums in ascending j
 *   N_i     = the sum of X_j over j != i           in ascending j
 *   masks_i = tf_mask(X_i, N_i)                    cfg.mask_type / mask_pow / mask_bin_thr_db, the arithmetic of disco_tf_mask
 * The reference transforms the time-domain sums instead; the transform is linear, so the two differ by rounding only.  Two sources
 * share one complex FFT (ceil(n_src / 2) transforms per frame, against 1 + 2 n_src of separate calls) and no spectrum but mix reaches
 * memory.  Per-room lengths (disco_set_lengths) as for disco_mask_oracle: signal g of n_sig belongs to room g / (n_sig / cfg.rooms), the
 * padding reflects at the room's own end, masks and mix are exact zeros in the frames a room does not have, no sample at or beyond a
 * room's length is read.  A signal's output bits do not depend on the rest of the batch.
 * DISCO_E_UNSUPPORTED, nothing written: n_src outside 2 <= n_src <= 8.  DISCO_E_ARG: a null images or masks, n_sig < 1. */
int disco_source_masks(disco_ctx* ctx, const float* images, int n_src, int64_t n_sig, float* masks, disco_c32* mix, disco_stream s);

/* Masked batch spatial covariance -- the loop nests tango.py:357-364 (step 1, P = M, Zs = Zn = NULL)
 * and tango.py:433-440 (step 2, P = M + K - 1).
 *   v_s(t,f) = [ m*X_k ; g_s*Zs_j (j<k) ; g_s*Zs_j (j>k) ],   Rss[f] = mean_t v_s v_s^H
 *   v_n(t,f) = [(1-m)*X_k ; g_n*Zn_j ...               ],   Rnn[f] = mean_t v_n v_n^H
 * with g_s = m, g_n = 1-m when mask_remote != 0 (mask_for_z='local', tango.py:416-418) and 1 otherwise.
 * X [R][K][T][F][M], mask [R][K][T][F], Zs/Zn [R][K][T][F] (row order = concatenate_signals, tango.py:142-155).
 * Rss, Rnn: disco_c32 [R][K][F][P][P].  Limits: M <= 8, P <= 32 (DISCO_E_UNSUPPORTED beyond, naming the limit).  17 <= P <= 32
 * (csrc/k_cov_wide.h) checks the scratch its partial sums need, G x chunks x F x P(P+1)/2 x 16 B, before it runs and refuses a batch
 * that does not fit with DISCO_E_UNSUPPORTED. */
int disco_cov_masked(disco_ctx* ctx, const disco_c32* X, const float* mask,
                     const disco_c32* Zs, const disco_c32* Zn, int mask_remote, int P,
                     disco_c32* Rss, disco_c32* Rnn, disco_stream s);

/* intern_filter(Rxx, Rnn, mu, type='gevd', rank=1) -- internal_formulas.py:56-73, batched:
 * top (algebraically largest) generalized eigenpair of each Hermitian pencil, Rnn positive definite, Rxx any Hermitian
 * matrix (Ryy - Rnn included): float64 Cholesky whitening + repeated squaring, solved again on a shifted matrix where Rxx
 * is indefinite.  Eigenvalue clamped to [eps, 1e6], w = q d/(d+mu) (Q^-1)[0,0], t1 = q (Q^-1)[0,0]; where every
 * eigenvalue is <= 0, d = eps and w ~ 0.  An exactly repeated top eigenvalue yields some vector of its eigenspace.
 * Rss, Rnn: [n_prob][P][P]  ->  w, t1: [n_prob][P]  (t1 may be NULL).  1 <= P <= 32 (17 <= P <= 32: one wave per pencil,
 * csrc/k_solve_wide.h, the same algorithm and guards). */
int disco_gevd_mwf_r1(disco_ctx* ctx, const disco_c32* Rss, const disco_c32* Rnn, int64_t n_prob, int P,
                      float mu, disco_c32* w, disco_c32* t1, disco_stream s);

/* intern_filter(Rxx, Rnn, mu, type='gevd', rank) for every kept rank -- internal_formulas.py:56-73, batched.
 * With Rnn = L L^H and C = L^-1 Rxx L^-H = V diag(d) V^H (float64 Cholesky whitening, then every eigenpair of C by cyclic complex
 * Jacobi in float64):
 *     w  = L00 L^-H sum_{i kept} f_i v_i conj(v_i[0]),   f_i = dc_i / (dc_i + mu),  dc_i = d_i clamped to [eps, 1e6]
 *     t1 = L00 L^-H v_top conj(v_top[0])   (the rank-1 t1, whatever the rank)
 * The pairs are ranked by their UNCLAMPED eigenvalue, descending, ties broken by index; the first min(rank, P) are kept.  rank >= P is
 * full rank, rank = 0 gives w = 0; a negative rank is DISCO_E_ARG (the reference's slicing rule, r = max(P + rank, 0), is the caller's).
 * mu = 0 with rank < P is the reference's singular inv(D + 0 I); here the dropped pairs simply contribute nothing.
 * A numerically singular Rnn takes the pivot floor of the rank-1 solver (its breakdown columns are zeroed): finite and bounded, with
 * the large eigenvalues it produces clamped to 1e6.  A pencil that is not finite returns non-finite w, t1 and leaves the other
 * pencils of the batch unchanged.
 * Rxx, Rnn: [n_prob][P][P] (Hermitian)  ->  w, t1: [n_prob][P]  (t1 may be NULL).  1 <= P <= 16 (rank 1 above 16: disco_gevd_mwf_r1). */
int disco_gevd_mwf(disco_ctx* ctx, const disco_c32* Rxx, const disco_c32* Rnn, int64_t n_prob, int P, int rank, float mu,
                   disco_c32* w, disco_c32* t1, disco_stream s);

/* intern_filter's other two branches (internal_formulas.py:45-54 'r1-mwf' -- the function's DEFAULT type -- and :74-76 'mwf');
 * neither is reached by offline_tango, both are here so that the whole function is:
 *   DISCO_FILTER_R1_MWF  Rxx1 = |Dmax| x x^H (top eigenpair of Rxx: Dmax its largest eigenvalue, as D.max());
 *                        P = Rnn^-1 Rxx1; w = P[:, 0] / (mu + trace P)
 *   DISCO_FILTER_MWF     w = ((Rnn + Rxx)^-1 Rxx)[:, 0]
 * Rxx, Rnn [n_prob][P][P] -> w [n_prob][P]; t1 of these branches is e_1 (internal_formulas.py:43), the caller's to fill. */
#define DISCO_FILTER_R1_MWF 1
#define DISCO_FILTER_MWF    2
int disco_mwf_filter(disco_ctx* ctx, const disco_c32* Rxx, const disco_c32* Rnn, int64_t n_prob, int P, float mu, int type,
                     disco_c32* w, disco_stream s);

/* The same solve, fed straight from the partial sums the LAST covariance call of this context left in its scratch
 * (any of disco_cov_masked / disco_stft_cov_fused / disco_step2_cov_fused; those accept Rss == Rnn == NULL when the
 * matrices themselves are not wanted).  Saves writing and re-reading the [R][K][F][P][P] matrices.
 * w, t1: [R][K][F][P] with the P of that covariance call (P <= 32). */
int disco_gevd_mwf_r1_pending(disco_ctx* ctx, float mu, disco_c32* w, disco_c32* t1, disco_stream s);

/* Filter-and-sum -- the np.inner loops tango.py:369-374 / 445-450:
 *   out[t,f] = sum_p c(w[f,p]) * v[p,t,f],  v = [X_k ; Z_j (j<k) ; Z_j (j>k)],  c = conj if conj_w else identity.
 * X [R][K][T][F][M]; Z [R][K][T][F] or NULL when P == M; w [R][K][F][P]; out [R][K][T][F].  M <= 8, P <= 32. */
int disco_apply(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const disco_c32* w, int P,
                int conj_w, disco_c32* out, disco_stream s);

/* zn = Y[ref_mic] - z_y -- tango.py:376.  X [R][K][T][F][M], z/zn [R][K][T][F]. */
int disco_noise_residual(disco_ctx* ctx, const disco_c32* X, const disco_c32* z, disco_c32* zn, disco_stream s);

/* STFT and step-1 covariance in one pass over the samples (tango.py:335 + 357-364): equivalent to
 * disco_stft(y, R*K, M) -> X ; disco_cov_masked(X, mask_z, NULL, NULL, 0, M) without re-reading X.
 * y [R][K][M][L], mask_z [R][K][T][F] -> X [R][K][T][F][M], Rss, Rnn [R][K][F][M][M]. */
int disco_stft_cov_fused(disco_ctx* ctx, const float* y, const float* mask_z, disco_c32* X,
                         disco_c32* Rss, disco_c32* Rnn, disco_stream s);

/* ---- step 2 with the z exchange in registers (all K nodes of a room on this GPU, mask_for_z = 'local') ------ */

/* tango.py:369 + 382-386 + 433-440 in one pass over X: every node's z_k = w_loc,k^H y_k is formed on the fly,
 * swapped between the K node-lanes of a bin with lane shuffles, and the (M+K-1)^2 masked covariances of every
 * node are accumulated.  Equivalent to disco_apply(X, w_loc) -> z ; disco_cov_masked(X, mask_w, z, z, 1, M+K-1).
 * X [R][K][T][F][M], mask_w [R][K][T][F], w_loc [R][K][F][M]; z_out [R][K][T][F] or NULL;
 * Rss, Rnn [R][K][F][P][P], P = M + K - 1 <= 8. */
int disco_step2_cov_fused(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc,
                          disco_c32* z_out, disco_c32* Rss, disco_c32* Rnn, disco_stream s);

/* The same pass when mask_w IS the step-1 mask (oracle masks; a DNN mask re-used, tango.py:388-389): the leading
 * M x M block of every node's step-2 covariance then equals its step-1 covariance, whose partial sums the preceding
 * disco_stft_cov_fused call left in this context; that block is neither accumulated nor written, and
 * disco_gevd_mwf_r1_pending assembles the pencil from both sets of partial sums.
 * Contract: the LAST covariance call of this context was disco_stft_cov_fused(y, mask_w, X, ...) producing THIS X with
 * THIS mask_w (only disco_gevd_mwf_r1_pending may have run in between); anything else returns DISCO_E_ARG.  The check is on
 * the POINTERS: the caller must not have rewritten X or mask_w in place since (the library cannot see that).
 * The matrices themselves are not available from this entry point (use disco_step2_cov_fused for Rss / Rnn). */
int disco_step2_cov_fused_reuse(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc,
                                disco_c32* z_out, disco_stream s);

/* tango.py:369 + 382 + 445 in one pass over X: yf_k = w_glo,k^H [y_k ; z_j (j<k) ; z_j (j>k)] with z recomputed
 * from w_loc.  Equivalent to disco_apply(X, w_loc) -> z ; disco_apply(X, z, w_glo, M+K-1).
 * w_glo [R][K][F][P]; yf [R][K][T][F]; z_out [R][K][T][F] or NULL. */
int disco_step2_apply_fused(disco_ctx* ctx, const disco_c32* X, const disco_c32* w_loc, const disco_c32* w_glo,
                            disco_c32* z_out, disco_c32* yf, disco_stream s);

/* disco_step2_apply_fused followed by disco_istft, without yf ever reaching HBM (tango.py:445 + 528-529): every
 * wave filters two frames of its node, packs them into one complex inverse FFT, overlap-adds and stores time samples.
 * out: float [R][K][L].  512-point STFT, M + K - 1 <= 8; DISCO_E_UNSUPPORTED otherwise (use the two calls). */
int disco_step2_apply_istft_fused(disco_ctx* ctx, const disco_c32* X, const disco_c32* w_loc, const disco_c32* w_glo,
                                  float* out, disco_stream s);

/* disco_apply(X, Z, w, P = M + K - 1, conj_w = 1) followed by disco_istft, in one pass with z taken from HBM (tango.py:445 + 528): what a
 * NODE SHARD ends its step 2 with -- its z rows come out of the all-gather, in the layout disco_set_z_blocks names -- and what the whole-path
 * calls of the wide shapes end in (stage "apply2_istft", csrc/k_fused.h k_apply_istft_wide).
 *   X [R][Kl][T][F][M], Z: the z of ALL nodes, w [R][Kl][F][P] -> out float [R][Kl][L]; yf [R][Kl][T][F] or NULL.
 * Built for 512 / 1024-point frames and (mics, nodes) in {8, 4} x {8, 6} + (8, 4), (8, 2), (4, 4), (4, 3), (4, 2); DISCO_E_UNSUPPORTED
 * otherwise (use the two calls). */
int disco_apply_istft_fused(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const disco_c32* w, disco_c32* yf,
                            float* out, disco_stream s);

/* ---- whole path -------------------------------------------------------------------------------------- */

/* offline_tango(y, ..., mask_for_z='local') restricted to the y branch ("enhanced" outputs), device resident:
 *   y       float [R][K][M][L]       mixture
 *   mask_z  float [R][K][T][F]       step-1 mask (oracle via disco_mask_oracle, or a DNN's output)
 *   mask_w  float [R][K][T][F]       step-2 mask (may alias mask_z)
 *   out     float [R][K][L]          iSTFT of the step-2 output yf            (tango.py:528)
 *   z_y     disco_c32 [R][K][T][F]   compressed signals, or NULL to keep them in the workspace
 *   yf      disco_c32 [R][K][T][F]   step-2 STFT-domain output, or NULL
 * workspace: device buffer of at least disco_workspace_bytes(ctx), or NULL to let the context allocate
 * (once, lazily) and keep it. */
int disco_tango_enhance(disco_ctx* ctx, const float* y, const float* mask_z, const float* mask_w,
                        float* out, disco_c32* z_y, disco_c32* yf,
                        void* workspace, size_t workspace_bytes, disco_stream s);

/* offline_tango(y, s, n, vads, mods, mask_for_z) with ALL nine outputs ("reference" outputs, tango.py:252-457), device
 * resident: the target / noise images s, n ride through the same filters as the mixture so that the result can be scored
 * (tango.py:541-593).  One call = the loop nests tango.py:326-450 in order; nothing returns to the host in between.
 *   y, s, n      float [R][K][M][L]
 *   mask_z_in    float [R][K][T][F] step-1 mask, or NULL: tf_mask(S, N, cfg.mask_type) at cfg.ref_mic     (tango.py:338-342)
 *   mask_w_in    float [R][K][T][F] step-2 mask, or NULL: tf_mask(S, N, cfg.mask_type) at channel 0        (tango.py:391-394)
 *                ('ivad' / DNN masks are computed by the caller -- disco_mask_ivad, the CRNN -- and passed in)
 *   mask_for_z   DISCO_MZ_*: what the remote rows of the step-2 statistics are (tango.py:343-348, 396-429)
 *   steps        1: step 1 only (get_z_signals.py:213-317); 3: both; 2: step 2 only, on the state a previous `steps = 1` call
 *                with the same y, s, n left in the SAME workspace (a DNN step-2 mask needs z before it can be computed); the
 *                context remembers that state and returns DISCO_E_ARG for steps = 2 when it is not there -- no steps = 1 call,
 *                other y / s / n / workspace pointers, or another whole-path call that used the workspace in between
 *   out          device pointers, each [R][K][T][F]; any of them may be NULL (not wanted)
 * workspace: at least disco_reference_workspace_bytes(ctx) (three STFTs, the exchanged rows, filters), or NULL to let the
 * context allocate and keep it. */
#define DISCO_MZ_LOCAL        0   /* remote rows = z_y under the RECEIVING node's mask (the default, tango.py:36)        */
#define DISCO_MZ_NONE         1   /* mask_for_z=None: z_y for Rss, zn for Rnn, unmasked       (tango.py:419-422)      */
#define DISCO_MZ_DISTANT      2   /* z_y under the SENDER's step-2 mask                       (tango.py:396-401)      */
#define DISCO_MZ_COMPRESSED   3   /* z_y under tf_mask(z_s, z_n) of the sender                (tango.py:402-405)      */
#define DISCO_MZ_ORACLE_REFS  4   /* oracle images at the reference mics; oracle statistics   (tango.py:343-345, 406) */
#define DISCO_MZ_ORACLE_ZS    5   /* z_s / z_n; oracle statistics at step 1                   (tango.py:408-409)      */
#define DISCO_MZ_PREVIOUS     6   /* any other string in the reference: unmasked z_y in both  (tango.py:428-429)      */
typedef struct disco_ref_outputs {
    disco_c32 *yf, *sf, *nf, *z_y, *z_s, *z_n, *zn;
    float *masks_z, *mask_w;
} disco_ref_outputs;
size_t disco_reference_workspace_bytes(const disco_ctx* ctx);
int disco_tango_reference(disco_ctx* ctx, const float* y, const float* s, const float* n, const float* mask_z_in,
                          const float* mask_w_in, int mask_for_z, int steps, const disco_ref_outputs* out,
                          void* workspace, size_t workspace_bytes, disco_stream st);

/* DANSE-style continuation of the two-step scheme (BASELINE.json configs[4]; NOT in the reference, which is strictly
 * two-step, tango.py:1-7): step 2 is run `iters` times, and between two runs every node re-compresses with the local part
 * of its new global filter, z_k <- w_glo,k[0:M]^H y_k.  iters = 1 gives exactly disco_tango_enhance's outputs.  Staged
 * kernels (z materialised), any P = M + K - 1 <= 32.  Arguments as disco_tango_enhance; z_y returns the LAST z. */
int disco_tango_enhance_iterated(disco_ctx* ctx, const float* y, const float* mask_z, const float* mask_w, int iters,
                                 float* out, disco_c32* z_y, disco_c32* yf,
                                 void* workspace, size_t workspace_bytes, disco_stream s);

/* w_loc[..][f][0:M] = w_glo[..][f][0:M]: the local part of every node's P-entry global filter -- the re-compression filter
 * of the iterated scheme above, exposed so that a node-sharded run (disco_set_node_shard) can iterate with one all-gather
 * of z per iteration.  w_glo [R][K][F][P] -> w_loc [R][K][F][M]  (K = the shard's node count when a shard is active). */
int disco_filter_head(disco_ctx* ctx, const disco_c32* w_glo, int P, disco_c32* w_loc, disco_stream s);

/* 'ivad' mask -- get_mask(..., mask_type='ivad', ts=s[node][0]) (tango.py:217-221): vad_oracle_batch (sigproc_utils.py:12-55:
 * window power test against 0.001 * the 0.99-quantile of the centred signal's instantaneous power, win = n_fft, hop) sampled
 * every hop and tiled over frequency; frames beyond ceil(L / hop) are 0.
 * s_ref [n_sig][L] (the target's time signal at channel 0) -> mask [n_sig][T][F] of 0.0 / 1.0.  L <= 4096 hops. */
int disco_mask_ivad(disco_ctx* ctx, const float* s_ref, int64_t n_sig, float* mask, disco_stream s);

/* ---- online / adaptive mode -----------------------------------------------------------------
 * The reference ships the smoothing primitive spatial_correlation_matrix (se_utils/internal_formulas.py:84-103:
 * R <- lambda R + M (1 - lambda) x x^H) and intern_filter (:56-73) but no loop around them; these entry points are
 * that loop, causal in t, per (room, node, bin):
 *     Rss_t = lambda Rss_{t-1} + (1-lambda) m_t v_t v_t^H ,        Rss_-1 = 0
 *     Rnn_t = lambda Rnn_{t-1} + (1-lambda) (1-m_t) v_t v_t^H ,    Rnn_-1 = init_diag I
 *     w_t   = intern_filter(Rss_t, Rnn_t, mu, 'gevd', rank=1)  when t % update_every == 0, else w_{t-1}
 *     out_t = w_t^H v_t ,   v_t = [X_k(t,f,:) ; Z_j(t,f) j<k ; Z_j(t,f) j>k]   (concatenate_signals, tango.py:142-155)
 * X [R][Kl][T][F][M]; Z [R][K][T][F] (all nodes; needed iff P = M + K - 1, ignored iff P = M); mask [R][Kl][T][F];
 * out [R][Kl][T][F]; w_last [R][Kl][F][P] or NULL (the filter in force at the last frame).
 * Routes by pencil size (csrc/api_online.hip; every one is launched by tests/test_gpu_online_sizes.py):
 *     P <= 4         one thread per (room, node, bin): k_online_mwf_thread<P>
 *     5 <= P <= 7    one thread per problem unless option "solve_thread" = 0, then the lane-group kernel
 *     8 <= P <= 16   a group of 8 (P = 8; also 5..7 on this route) or 16 lanes per problem: k_online_mwf<P>
 *     P > 16         DISCO_E_UNSUPPORTED
 * Option "online_sq32" applies to the thread route only.  P other than mics or mics + nodes - 1, P > mics without Z, lambda_cor
 * outside [0, 1), update_every < 1 or init_diag <= 0: DISCO_E_ARG, nothing written. */
int disco_online_mwf(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const float* mask, int P,
                     float lambda_cor, float mu, int update_every, float init_diag,
                     disco_c32* out, disco_c32* w_last, disco_stream s);

/* The two-step path in online mode: disco_stft -> disco_online_mwf(P = M) -> z -> disco_online_mwf(P = M + K - 1)
 * -> yf -> disco_istft.  Both steps are causal in t, so frame t of the output depends on frames <= t of the inputs
 * (plus the half-window look-ahead of the centred STFT).  Arguments as disco_tango_enhance; mu from the cfg. */
int disco_tango_online(disco_ctx* ctx, const float* y, const float* mask_z, const float* mask_w,
                       float lambda_cor, int update_every, float init_diag,
                       float* out, disco_c32* z_y, disco_c32* yf,
                       void* workspace, size_t workspace_bytes, disco_stream s);

/* ---- scoring the online mode: companions through the per-frame filters ---------------------------------------------------------------
 * Every score of the reference (tango.py:541-593) needs the target image and the noise image carried through the SAME filters as the
 * mixture.  Online the filter changes at every update, and a filter history for a second pass would be P times the size of the output,
 * so the companions ride through the walk itself: disco_online_mwf with one or two further inputs laid out as X / Z,
 *     out^c_t = w_t^H v^c_t ,   v^c_t = [X^c_k(t,f,:) ; Z^c_j(t,f) j<k ; Z^c_j(t,f) j>k] ,
 * w_t the filter in force at frame t.  Companions never enter Rss, Rnn or the solve: out and w_last are those of disco_online_mwf on
 * the same inputs, route and options, bit for bit, and a non-finite companion value stays in its own output at its own frame.
 * comp[i].X [R][Kl][T][F][M]; comp[i].Z [R][K][T][F] in the layout of Z (disco_set_z_blocks; needed iff P = M + K - 1);
 * comp[i].out [R][Kl][T][F].  Node shards as for disco_online_mwf.  Argument rules of disco_online_mwf; in addition DISCO_E_ARG for
 * n_comp other than 1 or 2, a companion without X or out, P > mics with a companion's Z missing.  A refusal writes nothing.
 * Kernels: k_online_mwf_thread_ref<P, SQ32> and k_online_mwf_ref<P> (csrc/k_online.h), on the routes of disco_online_mwf. */
typedef struct disco_online_companion {
    const disco_c32* X;
    const disco_c32* Z;
    disco_c32* out;
} disco_online_companion;
int disco_online_mwf_ref(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, const float* mask, int P,
                         float lambda_cor, float mu, int update_every, float init_diag,
                         disco_c32* out, disco_c32* w_last, const disco_online_companion* comp, int n_comp, disco_stream s);

/* disco_tango_reference's nine outputs in online mode (mask_for_z = 'local', the only mode the online recursion has): disco_stft of
 * y, s, n; the masks (NULL: the oracle TF mask of cfg.mask_type from S, N, at cfg.ref_mic for step 1 and at channel 0 for step 2);
 * online step 1 with companions -> z_y, z_s, z_n; zn = Y[ref] - z_y; online step 2 on [Y_k ; z_y,j] with companions [S_k ; z_s,j] and
 * [N_k ; z_n,j] -> yf, sf, nf.  The exchanged rows are complex64.  A single node under one mask: step 2 repeats step 1 and is skipped.
 *   out       device pointers, each [R][K][T][F]; any of them may be NULL (not wanted)
 *   time_out  float [6][R][K][L] or NULL: the inverse transforms of yf, sf, nf, z_y, z_s, z_n in that order -- the six signals the
 *             scores take
 *   workspace at least disco_online_reference_workspace_bytes(ctx), or NULL for the context's own (disco_reserve(ctx, 2) covers it)
 * With the workspace reserved the call allocates nothing and synchronises nothing: a fixed launch sequence that may be captured in a
 * graph.  DISCO_E_UNSUPPORTED: per-room lengths set, a node shard active, mics + nodes - 1 > 16.
 * Stage timers: stft, masks, online1_ref, online2_ref, istft. */
size_t disco_online_reference_workspace_bytes(const disco_ctx* ctx);
int disco_tango_online_reference(disco_ctx* ctx, const float* y, const float* s, const float* n, const float* mask_z_in,
                                 const float* mask_w_in, float lambda_cor, int update_every, float init_diag,
                                 const disco_ref_outputs* out, float* time_out,
                                 void* workspace, size_t workspace_bytes, disco_stream st);

/* The online two-step path as a STREAM -- state in, state out ("streaming latency instead of batch"; the reference's
 * primitive is a one-frame update, se_utils/internal_formulas.py:84-103).  One call consumes n_hops hops of NEW samples per channel and
 * emits every output sample that became final:
 *   y_new    float [R][K][M][n_hops * hop]   the next samples of every channel (hops_before * hop samples went before them)
 *   mask_z/w float [R][K][n_new][F]          masks of the frames this call completes, n_new = n_hops + (last ? 1 : 0): frame t (centred at
 *                                            sample t * hop) needs the samples up to t * hop + n_fft / 2, so h hops of input complete the
 *                                            frames 0 ... h - 1; `last` adds the frame centred at the end of the signal
 *   out      float [R][K][n_out]             n_out = hop * (n_new - (hops_before == 0 ? 1 : 0)): the samples between the centres of the
 *                                            frames completed so far are final -- the latency is one hop plus the chunk
 *   state    caller-owned device block of disco_online_state_bytes(ctx): the last hop of samples of every channel, the last output
 *            spectrum, both smoothed matrices (Hermitian: their lower triangles) and the filter in force of every (room, node, bin) of both
 *            steps.  Written by every call,
 *            read by every call but the first (hops_before == 0, which needs n_hops >= 2).  Nothing of a stream lives in the context:
 *            streams may be interleaved, moved between contexts of the same cfg, or checkpointed by copying the block.
 *   workspace at least disco_online_stream_workspace_bytes(ctx, n_hops)
 * The per-frame arithmetic is that of disco_tango_online (same kernels, on a transform block of the chunk's frames): N chunks reproduce one
 * whole-clip call bit for bit.  lambda_cor / update_every / init_diag as disco_online_mwf (filter updates fall on frames t % update_every
 * == 0 of the STREAM); mu from the cfg; cfg.length is not used. */
size_t disco_online_state_bytes(const disco_ctx* ctx);
size_t disco_online_stream_workspace_bytes(const disco_ctx* ctx, int max_hops);
int disco_tango_online_stream(disco_ctx* ctx, const float* y_new, int n_hops, const float* mask_z, const float* mask_w,
                              float lambda_cor, int update_every, float init_diag, int64_t hops_before, int last, void* state,
                              float* out, void* workspace, size_t workspace_bytes, disco_stream s);

/* ---- helper of the mask-estimation DNN, which otherwise stays in PyTorch-ROCm ------------------------------------
 * The pointwise half of one GRU step for n independent sequences (gate order r, z, n as torch.nn.GRU; the two matrix products
 * are the caller's GEMMs):  r = sigm(gi_r + gh_r), z = sigm(gi_z + gh_z), c = tanh(gi_n + r gh_n), h' = (1 - z) c + z h.
 *   gi      rows of 3H floats at stride gi_stride (floats): one time step of the all-steps input projection
 *   gh      [n][3H] = h W_hh^T + b_hh, or NULL together with gh_bias [3H] for the first step (h = 0)
 *   h_prev  [n][H] or NULL (= 0);  h_out [n][H] (may alias h_prev)
 * ctx may be NULL: the launch then goes to the calling thread's current device (the DNN owns no disco_ctx). */
int disco_gru_gates(disco_ctx* ctx, const float* gi, int64_t gi_stride, const float* gh, const float* gh_bias,
                    const float* h_prev, float* h_out, int64_t n, int H, disco_stream s);

/* ---- training the mask estimators (disco_amd/dnn/train.py; the reference's dnn/engine/train.py, dnn/utils.py:189-294, dnn/engine/losses.py,
 * dnn/data/datasets.py).  The convolutions, BatchNorm, the GEMMs and the optimiser stay in PyTorch-ROCm with its autograd; these five are the
 * recurrent layer's pointwise forward and backward, the loss with its gradient, and the batch gather.  ctx may be NULL in all of them.
 *
 * disco_gru_gates that also keeps what back-propagation needs: saved [n][4H] = [r | z | c | gh_n] (gh_n: the recurrent pre-activation of the
 * candidate gate, the value r multiplies; gh_bias's third block on the first step).  h_out holds the bits disco_gru_gates writes. */
int disco_gru_gates_train(disco_ctx* ctx, const float* gi, int64_t gi_stride, const float* gh, const float* gh_bias, const float* h_prev,
                          float* h_out, float* saved, int64_t n, int H, disco_stream s);

/* One step of back-propagation through time through disco_gru_gates_train.  With d = d_out + d_carry:
 *   dn = d (1 - z),  dz = d (h_prev - c),  d_h_direct = d z,  da_n = dn (1 - c^2),  da_z = dz z (1 - z),  da_r = da_n gh_n r (1 - r)
 *   d_out      rows of H floats at stride d_out_stride, or NULL: the gradient arriving at this step's output
 *   d_carry    [n][H] or NULL: the gradient carried from step t + 1 (not both NULL)
 *   saved      [n][4H] of this step;  h_prev [n][H] or NULL (= 0)
 *   d_gi       = [da_r | da_z | da_n], rows of 3H floats at stride d_gi_stride (a step's slice of an [n][steps][3H] buffer)
 *   d_gh       = [da_r | da_z | da_n r], [n][3H];  d_h_direct [n][H]
 * The caller's GEMMs finish the step: d_carry' = d_h_direct + d_gh W_hh, dW_hh += d_gh^T h_prev, db_hh += sum_rows d_gh. */
int disco_gru_gates_backward(disco_ctx* ctx, const float* d_out, int64_t d_out_stride, const float* d_carry, const float* saved,
                             const float* h_prev, float* d_gi, int64_t d_gi_stride, float* d_gh, float* d_h_direct, int64_t n, int H,
                             disco_stream s);

/* reconstruction_loss (dnn/engine/losses.py:4-25) on the frames get_x_for_loss selects (dnn/utils.py:212-246), without slicing them out:
 *   term(b, j, f) = ((est[b][j][f] - y[b][ff_in + j][f]) x[b][0][ff_in + j][f])^2,  j < n_out, ff_in + n_out <= W
 * est [B][n_out][F], label y [B][W][F], input x [B][C][W][F] (channel 0 weights the loss), all float32.  Every term is formed and summed in
 * float64; sums (device) receives {sum of the non-NaN terms, their count}, the loss is their quotient.  The order of summation is a function
 * of B n_out F alone (per-workgroup partial sums in `workspace`, one fold, no atomics): two calls give the same bits.
 * workspace: device memory, 8-byte aligned, DISCO_RECON_LOSS_WS_BYTES are always enough. */
#define DISCO_RECON_LOSS_MAX_BLOCKS 1024
#define DISCO_RECON_LOSS_WS_BYTES 16384
int disco_recon_loss(disco_ctx* ctx, const float* est, const float* y, const float* x, int64_t B, int C, int W, int F, int ff_in, int n_out,
                     double* sums, void* workspace, size_t workspace_bytes, disco_stream s);

/* Its gradient: d_est[b][j][f] = g 2 (est - y) x^2 / count, formed in float64 and rounded once to float32; g (the upstream gradient, one
 * float) and sums (what disco_recon_loss wrote) are read from device memory.  Exact +0 where the term is NaN -- the reference's autograd
 * leaves 0 x NaN = NaN there. */
int disco_recon_loss_grad(disco_ctx* ctx, const float* est, const float* y, const float* x, int64_t B, int C, int W, int F, int ff_in, int n_out,
                          const double* sums, const float* g, float* d_est, disco_stream s);

/* A training batch out of the spectra bank (DiscoDataset.get_subwindow, dnn/data/datasets.py:120-162): bank [S][N][T][F] float32 magnitudes (S
 * signal rows, N segments), tab (device) [B][C + 3] int32 = per item (segment k, first frame m, C input rows, label row) ->
 *   x[b][c] = bank[tab[b][2 + c]][k][m : m + W],  y[b] = bank[tab[b][2 + C]][k][m : m + W];   x [B][C][W][F], y [B][W][F].
 * tab_host: the caller's host copy of tab, or NULL.  Given, every entry is checked before the launch and an entry out of range (segment, m + W > T,
 * signal row) is DISCO_E_ARG.  The kernel itself never reads outside the bank: an item with such an entry comes out as zeros. */
int disco_train_batch(disco_ctx* ctx, const float* bank, int S, int64_t N, int T, int F, const int32_t* tab, const int32_t* tab_host, int64_t B,
                      int C, int W, float* x, float* y, disco_stream s);

/* The spectra bank filled from rooms without leaving the device: the rows of bank [S][N][Tb][F] (float32, what disco_train_batch reads) of the R
 * consecutive segments seg0 ... seg0 + R - 1, in one launch.  Sources, all on the device:
 *   X       [R][K][T][F][M] complex64 mixture spectra, read at microphone `mic` (M = 1: the plain [R][K][T][F])
 *   z0, z1  [R][K][T][F] complex64 compressed signals; either may be NULL, n_zsig is the number present (they keep their order)
 *   mask    [R][K][T][F] float32 labels;  frames [R] int32 or NULL (= T for every room; a value above T counts as T)
 * Rows (S = K (2 + n_zsig)): row k = |X| of node k, row K (1 + i) + k = |z signal i| of node k, row K (1 + n_zsig) + k = the mask of node k.
 * Frame tb of segment seg0 + r holds source frame tb + skip while tb + skip < min(frames[r], T) and an exact +0 for every other tb < Tb: all Tb
 * frames of the R segments are written, no other segment is touched, nothing is read out of range.  Magnitudes are
 * sqrtf(fmaf(re, re, im * im)), the bits disco_crnn_features gives before its clip (NaN passes); mask values are copied bit for bit.
 * DISCO_E_ARG, before anything is launched: X, mask or bank NULL, mic outside [0, M), skip < 0, Tb < 1, seg0 < 0, seg0 + R > N, n_zsig not
 * the number of z pointers.  ctx may be NULL. */
int disco_bank_fill(disco_ctx* ctx, const disco_c32* X, const disco_c32* z0, const disco_c32* z1, const float* mask, const int32_t* frames, int64_t R,
                    int K, int M, int T, int F, int mic, int n_zsig, int skip, float* bank, int64_t N, int Tb, int64_t seg0, disco_stream s);

/* MaxPool2d((1, 4)) of the CRNN's convolutional stack (dnn/models/crnn.py via nn_structures.py): floor-mode maximum over groups
 * of 4 along the last axis, plus the preceding convolution's per-channel bias (a constant commutes with the maximum; adding it here
 * spares a pass over the four times larger un-pooled map).  x [B][channels][rows_per_channel][row_len] seen as n_rows rows ->
 * out [n_rows][row_len / 4]; bias [channels] or NULL.  ctx may be NULL. */
int disco_maxpool_last4(disco_ctx* ctx, const float* x, const float* bias, int64_t n_rows, int row_len, int rows_per_channel,
                        int channels, float* out, disco_stream s);

/* First block of the CRNN's convolutional stack in one pass (dnn/models/crnn.py via nn_structures.py CNN2d): Conv2d(c_in -> c_out, 3x3,
 * padding (0, 1)) with the BatchNorm2d folded into w / bias by the caller, then MaxPool2d((1, 4)) (floor mode):
 *   out[b][o][t][q] = bias[o] + max_{j<4} sum_{c,kt,kf} w[o][c][kt][kf] x[b][c][t + kt][4 q + j + kf - 1]      (x = 0 outside [0, n_freq))
 * x [B][c_in][t_in][n_freq], w [c_out][c_in][3][3], bias [c_out] -> out [B][c_out][t_in - 2][n_freq / 4]; the un-pooled map is never written.
 * Direct form for the stack's FIRST block: c_in <= 8, c_out a multiple of 8 (of 32 beyond 32), n_freq <= 259, B <= 65535; other shapes:
 * DISCO_E_UNSUPPORTED (the caller keeps the library convolution + disco_maxpool_last4).  ctx may be NULL. */
int disco_conv3x3_pool4(disco_ctx* ctx, const float* x, const float* w, const float* bias, int64_t B, int c_in, int c_out, int t_in, int n_freq,
                        float* out, disco_stream s);

/* The networks' input features in one pass (speech_enhancement/utils.py:69-138 prepare_data; tango.py:338, 391, 158-186 get_z_for_mask 'zs_hat'):
 *   out [R K][C][pad_lo + T + pad_hi][F] float = clip(|.|, lo, hi), zeros in the padding rows (the reference pads after clipping), of
 *   channel 0: microphone `mic` of the node's own spectra X [R][K][T][F][M]; channels 1 ... K - 1 (Z != NULL, C = K: the step-2 network): the compressed
 *   signals Z [R][K][T][F] of the other nodes in node order.  Z == NULL: C = 1 (the step-1 network).  ctx may be NULL. */
int disco_crnn_features(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, int64_t R, int K, int M, int T, int F, int mic, int pad_lo, int pad_hi,
                        float lo, float hi, float* out, disco_stream s);

/* disco_crnn_features for a batch whose rooms differ in clip length (disco_set_lengths): frames [R] (device) holds T_r = 1 + L_r / hop <= T.  Rows
 * pad_lo + t with t < T_r hold the bits disco_crnn_features writes; every row with t >= T_r is an exact 0.f like the padding rows -- NOT clipped up to
 * `lo`: the reference pads zeros after the clip, which is what the room run alone at T_r sees there -- in channel 0 and in the |z| channels alike;
 * X and Z are not read there.  ctx may be NULL. */
int disco_crnn_features_rooms(disco_ctx* ctx, const disco_c32* X, const disco_c32* Z, int64_t R, int K, int M, int T, int F, int mic, int pad_lo,
                              int pad_hi, float lo, float hi, const int32_t* frames, float* out, disco_stream s);

/* The recurrent layer's input windows: the reference re-interprets every 15-frame window of the (C, frames, 4) feature map as a
 * (15, 256) sequence WITHOUT a transpose (dnn/models/crnn.py:59), so window t is the flattened block feat[:, t : t + W, :];
 * out[(b T + t)][0 : n_keep] = its leading n_keep floats (n_keep = 256 x GRU steps actually run, a multiple of 4).
 * feat [B][C][Tp][4] float, Tp >= T + W - 1; feat and out 16-byte aligned.  ctx may be NULL. */
int disco_crnn_windows(disco_ctx* ctx, const float* feat, int64_t B, int C, int Tp, int T, int W, int n_keep, float* out,
                       disco_stream s);

/* disco_crnn_windows for signals of different frame counts, compacted: signal b has frames_sig[b] <= T frames (device, [B]) and row0[b] (device, [B]) is
 * the exclusive prefix sum of frames_sig; out [n_rows][n_keep], row row0[b] + t (t < frames_sig[b]) = the bytes disco_crnn_windows writes to row
 * b T + t.  Nothing else is written; a row outside [0, n_rows) is skipped.  Same alignment and argument rules as disco_crnn_windows.  ctx may be NULL. */
int disco_crnn_windows_rooms(disco_ctx* ctx, const float* feat, int64_t B, int C, int Tp, int T, int W, int n_keep, const int32_t* frames_sig,
                             const int64_t* row0, float* out, int64_t n_rows, disco_stream s);

/* The inverse placement, for the output layer's rows: out [B][T][F], out[b][t] = rows[row0[b] + t] for t < frames_sig[b], exact zeros for the frames a
 * signal does not have; rows [n_rows][F].  One pass that writes EVERY element of out (16-byte stores when out is 16-byte aligned).  ctx may be NULL. */
int disco_crnn_expand_rows(disco_ctx* ctx, const float* rows, int64_t n_rows, int64_t B, int T, int F, const int32_t* frames_sig, const int64_t* row0,
                           float* out, disco_stream s);

/* ---- evaluation metrics right after the path --------------------------------------------------
 * Raw float64 moments behind disco_theque/metrics.py; the dB / clipping / weighting of a handful of numbers per signal
 * is host arithmetic (disco_amd/metrics.py).
 *
 * disco_pair_stats: for each of n_sig signal pairs a[i][start:stop], b[i][start:stop] (rows of `len` floats):
 *   stats[i][8] = { #(a != 0), sum a, sum a^2, #(b != 0), sum b, sum b^2, sum a b, stop - start }
 *   -> snr / delta_snr / sd (np.var of the non-zero samples, metrics.py:9-61) and si_sdr (:342-391). */
int disco_pair_stats(disco_ctx* ctx, const float* a, const float* b, int64_t n_sig, int64_t len, int start, int stop,
                     double* stats, disco_stream s);
/* disco_pair_stats_spans: the same with a span per signal -- rooms of different clip lengths in one launch.  stop: device array of
 * n_sig int32, clamped into [start, len]; NULL = len for every signal (the rule of disco_stoi).  Pair i is scored over
 * [start, stop[i]) and stats[i][7] = stop[i] - start; no sample at or beyond stop[i] is read (they may hold anything, NaN included).
 * Row i has the bits of disco_pair_stats on that pair alone with the scalar stop = stop[i]. */
int disco_pair_stats_spans(disco_ctx* ctx, const float* a, const float* b, int64_t n_sig, int64_t len, int start, const int32_t* stop,
                           double* stats, disco_stream s);

/* disco_band_stats: y_j = scipy.signal.lfilter(b[j], a[j], x[i][start:stop]) for every band j (zero initial state at
 * `start`), then stats[i][j][3] = { #(y_j != 0), sum y_j, sum y_j^2 } -- the per-band levels of fw_snr / fw_sd
 * (metrics.py:104-109, 256-260).  b, a: [n_bands][9] float64 (order-4 band-pass 'ba' coefficients, device memory). */
int disco_band_stats(disco_ctx* ctx, const float* x, int64_t n_sig, int64_t len, int start, int stop,
                     const double* b, const double* a, int n_bands, double* stats, disco_stream s);
/* disco_band_stats_gated: the same with fw_snr's `vad_tar` / `vad_noi` (metrics.py:63, 104-112): gate [n_sig][len] float, indexed like x;
 * a filtered sample enters the statistics where gate != 0 (np.var(s_f[vad != 0])) instead of where the sample itself is non-zero:
 * stats[i][j][3] = { #(gate != 0), sum y_j over them, sum y_j^2 over them }.  gate == NULL: disco_band_stats. */
int disco_band_stats_gated(disco_ctx* ctx, const float* x, const float* gate, int64_t n_sig, int64_t len, int start, int stop,
                           const double* b, const double* a, int n_bands, double* stats, disco_stream s);
/* disco_band_stats_spans: disco_band_stats (gate == NULL) or disco_band_stats_gated with a span per signal.  stop: device array of
 * n_sig int32, clamped into [start, len]; NULL = len for every signal.  Signal i is filtered and scored over [start, stop[i]): its
 * recurrence and its statistics end there, so the ringing of the band filters past the end of a clip is never scored, and neither x
 * nor gate is read at or beyond stop[i].  stats[i] has the bits of the scalar call on that signal alone with stop = stop[i]. */
int disco_band_stats_spans(disco_ctx* ctx, const float* x, const float* gate, int64_t n_sig, int64_t len, int start, const int32_t* stop,
                           const double* b, const double* a, int n_bands, double* stats, disco_stream s);

/* disco_seg_snr: the segmental SNR of disco_theque/metrics.py:131-173 for n_sig signal pairs s, n [n_sig][len] float.  Pair i is scored
 * over [start, stop[i]) (stop: device array of n_sig int32, clamped into [start, len]; NULL = len) as if sliced and scored alone; nothing
 * at or beyond stop[i] is read.  With L = stop[i] - start: windows m = 0 .. N_w - 1 cover [start + m win_hop, start + m win_hop + win_len),
 * N_w = (L - win_len) / win_hop + 1, 0 when L < win_len (whole windows only).  Per window and signal, in float64 on the float32 samples:
 * mean = sum x / win_len, var = sum (x - mean)^2 / win_len (two passes, as np.var), floored at 2.220446049250313e-16;
 * v_m = clip(10 log10(var_s / var_n), lo_db, hi_db); weight g_m = 1, or vad[i][start + m win_hop] with vad [n_sig][len] float (the value
 * itself, not a non-zero test).
 *   out[i][4] = { sum g_m v_m, sum g_m, N_w, number of windows with v_m at a clip bound }
 * The segmental SNR sum g v / sum g is host arithmetic.  One workgroup per pair: row i has the same bits whatever else is in the batch
 * and from run to run, and a NaN inside row i changes no bit of any other row.
 * DISCO_E_ARG, nothing written: win_len < 1, win_hop < 1, win_hop > win_len, lo_db >= hi_db, a null s, n or out, n_sig < 0, start outside
 * [0, len].  DISCO_E_UNSUPPORTED: win_len > DISCO_SEG_SNR_MAX_WIN (a wave keeps a window of both signals in registers between the two
 * passes), len > 2^31 - 1. */
#define DISCO_SEG_SNR_MAX_WIN 2048
int disco_seg_snr(disco_ctx* ctx, const float* s, const float* n, const float* vad, int64_t n_sig, int64_t len, int start,
                  const int32_t* stop, int win_len, int win_hop, float lo_db, float hi_db, double* out, disco_stream st);

/* ---- BSS-eval SDR / SIR / SAR (what tango.py:541-567 takes from mir_eval.separation.bss_eval_sources) ---------------
 * Restated from its definition (Vincent, Gribonval, Fevotte 2006): the estimate is projected on the flen delayed copies of
 * the target reference and on those of all nsrc references; every figure is a function of lag correlations only.
 *
 * disco_lag_corr: for each of n_pair signal pairs (rows of `len` floats) and every lag t in [lag_lo, lag_hi] (within +-511):
 *   out[i][t - lag_lo] = sum_n a[i][n] b[i][n + t]   over the n with n and n + t inside [start, stop)   (float64; the products
 *   of float32 samples are exact).  workspace: at least disco_lag_corr_workspace_bytes(ctx, n_pair, len, lag_hi - lag_lo + 1)
 *   (per-chunk partial sums, added in chunk order: bit-identical from run to run, and per pair whatever else is in the batch). */
size_t disco_lag_corr_workspace_bytes(const disco_ctx* ctx, int64_t n_pair, int64_t len, int n_lag);
int disco_lag_corr(disco_ctx* ctx, const float* a, const float* b, int64_t n_pair, int64_t len, int start, int stop, int lag_lo,
                   int lag_hi, double* out, void* workspace, size_t workspace_bytes, disco_stream s);
/* disco_lag_corr_spans: the same with a span per pair.  stop: device array of n_pair int32, clamped into [start, len]; NULL = len for
 * every pair.  Both signals of pair i count as zero outside [start, stop[i]) and are not read there.  The partial sums are laid out for
 * the longest span (len - start: the same workspace size) and added in the same chunk order, a chunk past a pair's stop adding zeros:
 * out[i] has the bits of disco_lag_corr on that pair alone with stop = stop[i]. */
int disco_lag_corr_spans(disco_ctx* ctx, const float* a, const float* b, int64_t n_pair, int64_t len, int start, const int32_t* stop,
                         int lag_lo, int lag_hi, double* out, void* workspace, size_t workspace_bytes, disco_stream s);

/* disco_bss_eval: refs [n_set][nsrc][len], ests [n_set][n_est][nsrc][len] float (the n_est estimate sets of a reference set
 * share its factorisation), scored over [start, stop) with a flen-tap filter; 1 <= nsrc <= 4, 1 <= flen <= 512
 * (DISCO_E_UNSUPPORTED beyond).  With G the (nsrc flen)^2 block-Toeplitz Gram matrix of the delayed references and d its
 * right-hand side for an estimate e:  p_j = d_j^T G_jj^-1 d_j,  p_all = d^T G^-1 d,  ee = sum e^2, and
 *   all_pairs == 0: out[n_set][n_est][nsrc][4]        estimate i against source i
 *   all_pairs != 0: out[n_set][n_est][nsrc][nsrc][4]  estimate i against source j
 * each { p_j, p_all, ee, status }.  SDR = 10 log10(p_j / (ee - p_j)), SIR = 10 log10(p_j / (p_all - p_j)),
 * SAR = 10 log10(p_all / (ee - p_all)) are host arithmetic (disco_amd/metrics.py).  status[n_set] (int32) != 0, and the
 * set's energies NaN: a pivot of the Cholesky factorisation fell to or below N 2.2e-16 times its own diagonal entry of G --
 * a reference all zero, references linearly dependent, or G singular to working precision (mir_eval falls back to lstsq
 * there; this does not).  Other sets of the batch are unaffected.  workspace: at least
 * disco_bss_workspace_bytes(ctx, n_set, nsrc, flen, len): per set 8 (N0^2 + (nsrc - 1) N1^2) bytes of factors (N0, N1 = nsrc flen,
 * flen rounded up to 32) -- 10 MB for two sources at flen 512 -- plus the correlations and their per-chunk partial sums. */
size_t disco_bss_workspace_bytes(const disco_ctx* ctx, int64_t n_set, int nsrc, int flen, int64_t len);
int disco_bss_eval(disco_ctx* ctx, const float* refs, const float* ests, int64_t n_set, int nsrc, int n_est, int64_t len, int start,
                   int stop, int flen, int all_pairs, double* out, int32_t* status, void* workspace, size_t workspace_bytes,
                   disco_stream s);
/* disco_bss_eval_spans: the same with a span per reference set.  stop: device array of n_set int32, clamped into [start, len]; NULL =
 * len for every set.  The references of set i and all its estimates are scored over [start, stop[i]) and not read outside it; the
 * set's energies have the bits of disco_bss_eval on that set alone with stop = stop[i].  An empty span (stop[i] <= start) is an all-zero
 * reference: status[i] != 0 and NaN energies.  Same workspace; the batch-size limit is taken from len - start. */
int disco_bss_eval_spans(disco_ctx* ctx, const float* refs, const float* ests, int64_t n_set, int nsrc, int n_est, int64_t len, int start,
                         const int32_t* stop, int flen, int all_pairs, double* out, int32_t* status, void* workspace, size_t workspace_bytes,
                         disco_stream s);

/* disco_bss_estimates: the three estimate sets tango.py:547-549 scores per node, formed on the device from the mixture y, the step-2
 * output sh and the step-1 output szh, each [n_sig][len] float:
 *   ests[n_sig][3][2][len] = { {sh, y - sh}, {szh, y - szh}, {y, y - sh} }
 * with every difference (float)((double)a - (double)b): formed in float64 and rounded to float32 once.  stop: device array of n_sig
 * int32, clamped into [start, len]; NULL = len.  Samples outside [start, stop[i]) are written as exact zeros and not read.  This is the
 * `ests` argument of disco_bss_eval for n_sig reference sets (n_est = 3, nsrc = 2), and, for n_sig = R K, read as [R][3 K][2][len], the one
 * for R reference sets of 3 K estimate sets each (the `_dry` keys: one dry pair per room). */
int disco_bss_estimates(disco_ctx* ctx, const float* y, const float* sh, const float* szh, int64_t n_sig, int64_t len, int start,
                        const int32_t* stop, float* ests, disco_stream s);

/* ---- STOI (what tango.py:569-578 takes from pystoi.stoi) ------------------------------------------------------------
 * Restated from its definition (Taal, Hendriks, Heusdens, Jensen 2011) with pystoi's constants and conventions; the extended
 * measure is disco_estoi below.  x [n_pair][len] clean, y [n_pair][len] processed, float; pair i is scored over [start, stop[i]) (stop: device array
 * of n_pair int32, clamped into [start, len]; NULL = len for every pair).  p / q = 10000 / fs_sig in lowest terms; p == q: the
 * signals are at 10 kHz already and taps is not read.  Otherwise taps [n_taps] float64 (device memory, n_taps = 2 L + 1 odd, at
 * most 65536 -- DISCO_E_UNSUPPORTED beyond) is the normalised anti-aliasing filter h of pystoi's resample_oct and both signals
 * are resampled as scipy.signal.resample_poly(x, p, q, window = h): out[m] = p sum_i h[m q + L - p i] x[i], ceil(n p / q) samples.
 * Then: frames of 256 samples at hop 128 windowed by hanning(258)[1:-1]; the frames of x within 40 dB of its loudest are kept
 * (the same frames of y), overlap-added, framed and windowed again, transformed (512 points), summed over 15 third-octave bands
 * from 150 Hz; every run of 30 frames of every band is normalised, clipped at -15 dB SDR, centred and correlated.
 *   out[i][2] = { d, number of kept frames };  status[i] (int32): 0 scored; 1 fewer than 30 frames after the removal, d = 1e-5
 *   (pystoi warns and returns that); 2 the span gives no frame at all (fewer than 257 samples at 10 kHz), d = NaN.
 * An all-zero x gives d = 0.  A pair's result is bit-identical from run to run and whatever else is in the batch (no atomics).
 * workspace: at least disco_stoi_workspace_bytes(ctx, n_pair, len, p, q, n_taps) -- the two resampled signals (8 ceil(len p / q)
 * bytes per pair, none at 10 kHz), frame energies and indices, the band spectra (120 bytes per frame) and partial sums;
 * 0 for a shape disco_stoi refuses. */
size_t disco_stoi_workspace_bytes(const disco_ctx* ctx, int64_t n_pair, int64_t len, int p, int q, int n_taps);
int disco_stoi(disco_ctx* ctx, const float* x, const float* y, int64_t n_pair, int64_t len, int start, const int32_t* stop, int p, int q,
               const double* taps, int n_taps, double* out, int32_t* status, void* workspace, size_t workspace_bytes, disco_stream s);

/* ---- ESTOI (extended STOI: Jensen, Taal 2016; what pystoi computes with extended=True) -------------------------------
 * The arguments, the resampling, the kept frames, the 15 third-octave envelopes X, Y (15 x T), out[i][2], the status values, the
 * refusals and their codes are those of disco_stoi; the last stage differs.  With J = T - 29 segments and Xm = X[:, m : m + 30], Ym
 * alike, in float64: every row of Xm, Ym minus its mean over the 30 frames, divided by (its norm + EPS); every column of the
 * row-normalised matrices minus its mean over the 15 bands, divided by (its norm + EPS); d_m = sum(Xn o Yn) / 30; d = sum_m d_m / J.
 * EPS = 2.220446049250313e-16.  No clipping.  Restated from the definition, as STOI is.  pystoi adds EPS randn to the matrices
 * before each normalisation so that it never divides by zero; that jitter is NOT reproduced (it moves d by some 1e-15): the result
 * is deterministic and a row or column whose centred norm is exactly 0 contributes 0.  An all-zero x gives d = 0.  A pair's result
 * is bit-identical from run to run and whatever else is in the batch (no atomics).
 * workspace: at least disco_estoi_workspace_bytes(ctx, n_pair, len, p, q, n_taps); 0 for a shape disco_estoi refuses. */
#define DISCO_ESTOI_SEGS 64 /* segments of 30 frames one workgroup of the last stage owns */
size_t disco_estoi_workspace_bytes(const disco_ctx* ctx, int64_t n_pair, int64_t len, int p, int q, int n_taps);
int disco_estoi(disco_ctx* ctx, const float* x, const float* y, int64_t n_pair, int64_t len, int start, const int32_t* stop, int p, int q,
                const double* taps, int n_taps, double* out, int32_t* status, void* workspace, size_t workspace_bytes, disco_stream s);
/* disco_estoi_bands: the last stage of ESTOI alone, on envelopes computed elsewhere.  tob_x, tob_y [n_pair][15][tmax] float (device
 * memory; clean, processed); frames: device array of n_pair int32, pair i has T = frames[i] frames, clamped into [0, tmax]; NULL =
 * tmax for every pair.  Nothing at or beyond a pair's T is read.  out[i][2] = { d, T };  status[i]: 0 scored; 1 T < 30, d = 1e-5.
 * A NaN in a pair's envelopes makes that pair's d NaN and touches no other pair.  The bits of a pair are those disco_estoi gives for
 * the same envelopes, alone or in any batch.  workspace: at least 8 n_pair ceil(max(tmax - 29, 0) / DISCO_ESTOI_SEGS) bytes (one
 * partial sum per workgroup); may be NULL when that is 0. */
int disco_estoi_bands(disco_ctx* ctx, const float* tob_x, const float* tob_y, int64_t n_pair, int tmax, const int32_t* frames, double* out,
                      int32_t* status, void* workspace, size_t workspace_bytes, disco_stream s);

/* ---- the step before the path: reverberation of dry signals ------------------------------------
 * out[i][c][0:out_len] = np.convolve(dry[i], rir[i][c])[:out_len]  (zero beyond dry_len + rir_len - 1), the operation of
 * dataset_generation/gen_disco/convolve_signals.py:160-163 (and of pyroomacoustics' room.simulate, :94-97), batched:
 * dry [n_sig][dry_len], rir [n_sig][n_ch][rir_len] -> out [n_sig][n_ch][out_len].  rir_len <= 8192.
 * Partitioned overlap-save with 1024-point wave FFTs; the spectra workspace lives in the context. */
int disco_rir_convolve(disco_ctx* ctx, const float* dry, const float* rir, int64_t n_sig, int n_ch,
                       int dry_len, int rir_len, float* out, int out_len, disco_stream s);

/* ---- how reverberant a room came out: DRR and SRR (disco_theque/metrics.py:176-208) -------------------------------------------
 * disco_rir_split: for each of n_rir impulse responses rir [n_rir][rir_len] float,
 *   split[i] = min(argmax(rir[i]) + n_direct, rir_len)   (int32; np.argmax of the SIGNED response: the first of equal maxima, and a NaN
 *   wins at its first index);  energy[i][2] = { sum rir[i][:split]^2, sum rir[i][split:]^2 } in float64 (the squares are exact), added
 *   in a fixed order.  DRR = 10 log10(energy[0] / energy[1]) is host arithmetic.  One workgroup per response: a NaN stays in its row.
 * DISCO_E_ARG, nothing written: a null pointer, n_rir < 0, rir_len < 1, n_direct < 0.  DISCO_E_UNSUPPORTED: rir_len > 8192.
 *
 * disco_reverb_energies: dry [n_sig][dry_len], rir [n_sig][n_ch][rir_len], split [n_sig][n_ch] int32 (device memory; a value outside
 * [0, rir_len] is clamped into it) ->
 *   energy[i][c][2] = { sum np.convolve(dry[i], rir[i][c][:split])^2, sum np.convolve(dry[i], rir[i][c][split:])^2 }   (float64)
 * over the FULL convolutions (dry_len + rir_len - 1 samples); an empty side gives an exact 0.  SRR = 10 log10(energy[0] / energy[1]).
 * The partitioned overlap-save of disco_rir_convolve (its arithmetic, its spectra workspace in the context) with two accumulator sets
 * per output block and no output store: neither convolution is written to memory, and neither is formed as a difference.  A row's bits
 * depend on nothing else in the batch, and a NaN in one response or one dry signal reaches only its own rows.
 * DISCO_E_ARG, nothing written: a null pointer, n_sig < 0, n_ch < 1, dry_len < 1, rir_len < 1.  DISCO_E_UNSUPPORTED: rir_len > 8192. */
#define DISCO_REVERB_MAX_RIR 8192
int disco_rir_split(disco_ctx* ctx, const float* rir, int64_t n_rir, int rir_len, int n_direct, int32_t* split, double* energy,
                    disco_stream s);
int disco_reverb_energies(disco_ctx* ctx, const float* dry, const float* rir, const int32_t* split, int64_t n_sig, int n_ch, int dry_len,
                          int rir_len, double* energy, disco_stream s);

/* Shoebox image-source room impulse responses -- what the reference takes from pyroomacoustics
 * (dataset_generation/gen_disco/convolve_signals.py:243-246 pra.ShoeBox(dims, fs, max_order=20, absorption); :94-95
 * image_source_model + compute_rir).  Third-party, absent, unpinned: restated from Allen & Berkley (1979) with that
 * package's documented conventions (images with |nx|+|ny|+|nz| <= max_order, sqrt(1 - absorption) per reflection,
 * 1 / (4 pi d), 81-tap Hann-windowed sinc fractional delays, response shifted by 40 samples).
 * room_dims [n_room][3] (m), absorption [n_room], src [n_room][n_src][3], mic [n_room][n_mic][3]
 *   -> rir [n_room][n_src][n_mic][rir_len] (truncated at rir_len <= 8192).  Feeds disco_rir_convolve directly. */
int disco_ism_rir(disco_ctx* ctx, const float* room_dims, const float* absorption, const float* src, const float* mic,
                  int64_t n_room, int n_src, int n_mic, int max_order, float fs, float c_sound,
                  float* rir, int rir_len, disco_stream s);

/* ---- from reverberated sources to rooms: the per-sample VAD of the images and the scaled mix -----------------------
 * disco_vad_samples: vad_oracle_batch (sigproc_utils.py:12-55; get_convolved_vads, convolve_signals.py:102-115) for a batch, one
 * decision per SAMPLE.  x [n_sig][len] -> vad [n_sig][len] of exact 0.f / 1.f.  stop: device array of n_sig int32, clamped into
 * [0, len], or NULL (= len).  Signal i is processed as if it had been sliced to L_i = stop[i] and run alone: nothing at or beyond L_i
 * is read (NaN may sit there), vad is exact zeros at and beyond L_i, L_i == 0 gives all zeros and reads nothing.
 * Arithmetic (that of disco_mask_ivad, whose decision at frame t is vad[t * win_hop]): mean accumulated in float64 and rounded to
 * float32; x2 = |(x - mean)^2| in float32; threshold thr * the 0.99-quantile of x2 with NumPy's linear interpolation (radix select);
 * #(x2 > threshold) per hop segment.  Window n covers [n win_hop, min(n win_hop + win_len, L)) for n < N_w = ceil((L - win_len) /
 * win_hop + 1) (0 when that is <= 0: L <= win_len - win_hop has no window and an all-zero VAD, as the reference); it is active iff its
 * count >= N_ / rat (integer division, N_ its clipped length); a sample is 1 iff an active window covers it.
 * DISCO_E_ARG, nothing written: win_len < 1, win_hop < 1, win_len % win_hop != 0, rat < 1, thr negative or not finite, a null x or
 * vad, n_sig < 0.  DISCO_E_UNSUPPORTED: len > 4096 * win_hop (the hop counters live in LDS).  One workgroup per signal: row i has the
 * same bits whatever else is in the batch, and a NaN inside signal i changes no bit of any other row. */
int disco_vad_samples(disco_ctx* ctx, const float* x, int64_t n_sig, int64_t len, const int32_t* stop, int win_len, int win_hop,
                      float thr, int rat, float* vad, disco_stream s);

/* disco_mix_scaled: the noise scaled by a gain and mixed in, in one pass (the last line of increase_to_snr, sigproc_utils.py:212, 223;
 * PostGenerator.mix_sigs, dataset_utils/post_generator.py:103-113).  s [n_sig][len], n [n_sig][n_len] with n_len <= len (the reference
 * adds a shorter noise into a zero buffer); gain: device float, one per `group` consecutive signals (one gain per room serves all its
 * channels; group = 1: one per signal), n_sig % group == 0; stop as above, L_i = stop[i].
 *   n_out[i][t] = gain[i / group] * n[i][t]  for t < min(n_len, L_i), exact zero elsewhere in [0, len)
 *   y_out[i][t] = s[i][t] + n_out[i][t]      for t < L_i,             exact zero elsewhere
 * y_out is the sum with the ROUNDED product stored in n_out (no fused multiply-add): y_out - s == n_out.  n_out or y_out may be NULL,
 * not both; s may be NULL iff y_out is.  n_out == n (in place) is allowed when n_len == len.  Nothing of s or n at or beyond L_i is
 * read.  16-byte accesses when len and n_len are multiples of 4 and every array is 16-byte aligned, one float at a time otherwise. */
int disco_mix_scaled(disco_ctx* ctx, const float* s, const float* n, int64_t n_sig, int64_t len, int64_t n_len, const float* gain,
                     int group, const int32_t* stop, float* n_out, float* y_out, disco_stream st);

/* disco_source_mix: a meeting room of n_src talkers per channel, in one pass over the images (simulate_room,
 * dataset_generation/gen_meetit/convolve_signals.py:140-148: node k listens to talker k, all others are its noise).
 * images [n_src][n_row][len], source-major, row = room * n_mic + channel; target: HOST array of n_mic int32, target[c] in [0, n_src)
 * the talker of channel c (read during the call; at most 64 channels); stop: device array of n_row int32 or NULL, as for
 * disco_mix_scaled.  Each output [n_row][len], any may be NULL but not all:
 *   y_out[i] = ((images[0][i] + images[1][i]) + images[2][i]) + ...
 *   s_out[i] = images[target[i % n_mic]][i]
 *   n_out[i] = the sum of images[j][i] over j != target[i % n_mic], in ascending j
 * below L_i = stop[i], exact zeros at and beyond it, where nothing of images is read.  Plain float32 additions in exactly that order
 * (the results equal NumPy's float32 sums bit for bit).  16-byte accesses when len is a multiple of 4 and every array is 16-byte
 * aligned, one float at a time otherwise.
 * DISCO_E_UNSUPPORTED, nothing written: n_src outside 2 <= n_src <= 8, n_mic > 64.  DISCO_E_ARG: a target outside [0, n_src), n_row no
 * multiple of n_mic, a null images or target, no output. */
int disco_source_mix(disco_ctx* ctx, const float* images, int n_src, int64_t n_row, int64_t len, const int32_t* target, int n_mic,
                     const int32_t* stop, float* y_out, float* s_out, float* n_out, disco_stream st);

/* ---- dry sources: speech-shaped noise and the levelling pass (dataset_utils/signal_setups.py:42-138) ---------------
 * disco_noise_from_signal: noise_from_signal (sigproc_utils.py:257-279) for a batch -- noise with the magnitude spectrum of the signal
 * and the phases the caller drew.  x [n_sig][len]; stop: device array of n_sig int32 or NULL (= len), L_i = stop[i] clamped into
 * [0, min(len, n_fft)]; phase [n_sig][n_fft / 2 + 1] float32 in TURNS, in [0, 1) -- the reference's np.random.random(X.shape[-1]);
 * out [n_sig][len].  Per signal, with NumPy's conventions:
 *   X = rfft(x_i[:L_i], n_fft) (zero-padded);  Y_k = |X_k| (cos 2 pi u_k + i sin 2 pi u_k);  out_i[:L_i] = irfft(Y, n_fft)[:L_i]
 * (the imaginary parts of Y_0 and Y_{n_fft/2} do not enter, the scale is 1 / n_fft); out_i is exact zeros in [L_i, len).  Nothing of
 * x_i at or beyond L_i is read (NaN may sit there); L_i == 0 writes zeros and reads nothing.  u is reduced in turns before the sine
 * and cosine are taken (sincospif(2 u)), so the error of the factor does not grow with the angle.
 * n_fft = 2^p, 10 <= p <= 22 (513 samples to 262 s at 16 kHz); any other power of two: DISCO_E_UNSUPPORTED.  DISCO_E_ARG, nothing
 * written: n_fft no power of two, n_fft < len while stop is NULL, a null x, phase or out, n_sig < 0.
 * The transform is a multi-pass Stockham schedule over the half-length complex signal x[2 n] + i x[2 n + 1], its radices the 512- and
 * 1024-point wave transforms and register DFTs of 4, 8, 16 (disco_amd/csrc/k_sources.h); its twiddles come from a float64 table the
 * context caches per n_fft, its two complex planes (8 n_fft bytes per signal) are the context's own and lazy: the first call for a
 * new n_fft or a larger batch allocates and uploads, every later call is a fixed sequence of launches.  No atomics: row i has the
 * same bits whatever else is in the batch, and a NaN in row i changes no bit of another row. */
int disco_noise_from_signal(disco_ctx* ctx, const float* x, int64_t n_sig, int64_t len, const int32_t* stop, int64_t n_fft,
                            const float* phase, float* out, disco_stream s);

/* disco_affine_segment: subtract, scale, shift, wrap in one launch -- the levelling of get_target_segment (signal_setups.py:54-69:
 * start = 0, lead = fs) and the rolled, de-meaned cut of _read_random_signal (:133-136: np.roll(sig, len - rnd_start)[:n] is
 * sig[(rnd_start + t) mod len], lead = 0).  x [n_sig][len] -> out [n_sig][out_len]; L_i = stop[i] clamped into [0, len];
 *   out[i][lead + t] = (float)(((double)x[i][(start_i + t) mod L_i] - mean_i) * gain_i)    for 0 <= t < min(count_i, out_len - lead)
 * and exact zeros everywhere else in [0, out_len).  stop, start, count: device int32 per signal, mean, gain: device float64 per
 * signal; NULL stands for L_i = len, start = 0, count = L_i, mean = 0, gain = 1.  start is taken mod L_i, a negative count as 0;
 * count_i > L_i repeats the signal periodically; L_i == 0 gives zeros and reads nothing.  The subtraction and the product are each
 * rounded in float64, then once to float32.  DISCO_E_ARG, nothing written: lead < 0 or lead > out_len, a null x or out, n_sig < 0.
 * 16-byte accesses when len and out_len are multiples of 4 and both arrays are 16-byte aligned (a quad of sources that is not one
 * aligned run is still read by element), one float at a time otherwise. */
int disco_affine_segment(disco_ctx* ctx, const float* x, int64_t n_sig, int64_t len, const int32_t* stop, const int32_t* start,
                         const int32_t* count, const double* mean, const double* gain, int lead, float* out, int64_t out_len,
                         disco_stream s);

/* ---- self-test of the packed complex arithmetic the FFT / covariance / filter kernels are written on ---------------
 * (disco_amd/csrc/pk.h: v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 with op_sel / neg modifiers; no reference counterpart --
 * it pins the instruction encodings against their C++ statement, which is what the CPU-side kernel tests execute.)
 * a, b, c: [n] complex64 operands -> out_hw, out_ref: [n][DISCO_PK_SELFTEST_OPS] complex64, the same operations through
 * the instruction forms and through plain C++.  ctx may be NULL. */
/* Streaming kernel of known traffic with ONE dword per lane and instruction -- the access width of the STFT kernels' sample reads --
 * for calibrating HBM traffic counters (no reference counterpart): write != 0 copies src[0:n] to dst[0:n] (4n bytes read, 4n written);
 * write == 0 only reads (dst needs >= 4096 floats and is practically never written). */
int disco_selftest_stream(disco_ctx* ctx, const float* src, float* dst, int64_t n, int write, disco_stream s);

/* Self-test of the float64 cross-lane forms the 9 <= P <= 16 solver is written on (disco_amd/csrc/dpp64.h: v_fmac_f64 / v_mov_b64 with
 * DPP row_newbcast inside inline asm; no reference counterpart): a, b: [n] complex128 operands (n a multiple of 64; lane i of a
 * 16-lane row reads the operands of the other lanes of its row) -> out_hw, out_ref: [n][DISCO_DPP_SELFTEST_OPS] complex128, the same
 * operations through the instruction forms and through __shfl + plain fused multiply-adds.  Bit equality is what is asserted. */
#define DISCO_DPP_SELFTEST_OPS 8
int disco_selftest_dpp(disco_ctx* ctx, const double* a, const double* b, int64_t n, double* out_hw, double* out_ref, disco_stream s);

/* Self-test of the asm primitives of the persistent room pass (disco_amd/csrc/k_room.h; no reference counterpart): the LDS-DMA loads
 * (global_load_lds_dwordx4 / _dword behind the M0 save / set / restore) + the wait for them against plain loads, and the lane-level
 * 2 x 2 transposes (v_permlane32_swap / v_permlane16_swap + add, on float32 and on float64 values) against their __shfl_xor statement.  src: [n] float, n a multiple of
 * 256 -> out_hw, out_ref: [n / 4][DISCO_ROOM_SELFTEST_OPS] float (one row per lane).  Bit equality is what is asserted.  ctx may be NULL. */
#define DISCO_ROOM_SELFTEST_OPS 6
int disco_selftest_room(disco_ctx* ctx, const float* src, int64_t n, float* out_hw, float* out_ref, disco_stream s);

/* The kernels of the "packed_x" layout one by one (tests; no reference counterpart).  X here -- and only here -- is the PACKED array
 * [R][K][T][F - 1][M] complex64, slot 0 of a channel = (Re X[0], Re X[F - 1]); everything else is as in the call named.  512-point STFT.
 *   disco_selftest_stft_cov_packed    disco_stft_cov_fused writing X packed (it keeps the step-1 sums for X / mask_z like that call)
 *   disco_selftest_step2_cov_packed   reuse == 0: disco_step2_cov_fused reading X packed; reuse != 0: disco_step2_cov_fused_reuse (Rss, Rnn
 *                                     must be NULL; solve with disco_gevd_mwf_r1_pending).  nodes >= 2 */
int disco_selftest_stft_cov_packed(disco_ctx* ctx, const float* y, const float* mask_z, disco_c32* X, disco_c32* Rss, disco_c32* Rnn,
                                   disco_stream s);
int disco_selftest_step2_cov_packed(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc, disco_c32* z_out,
                                    disco_c32* Rss, disco_c32* Rnn, int reuse, disco_stream s);

/* The staged step 2 of the whole-path calls on the CALLER's spectra, and the matrices of whatever pencil is pending (tests; no reference
 * counterpart).  The persistent room pass (csrc/k_room.h) and the split kernels that skip the step-1 block are otherwise reached only from
 * time signals through disco_tango_enhance*, and leave a pencil the solver assembles from two sets of partial blocks, which
 * disco_cov_masked / disco_step2_cov_fused never hand out.
 *   disco_selftest_staged_step2     step 1 on X [R][K][T][F][M] with mask [R][K][T][F] (what disco_cov_masked(X, mask, P = M, NULL, NULL)
 *                                   runs: it keeps the step-1 sums of X / mask), then exactly what the whole-path calls run for the
 *                                   exchange + step-2 statistics with the same mask and the filters w_loc [R][K][F][M]: z [R][K][T][F]
 *                                   (room pass: written only when store_z != 0) and the step-2 pencil left pending for
 *                                   disco_gevd_mwf_r1_pending.  *route_out (may be NULL): DISCO_STAGED_ROUTE_ROOM the room pass,
 *                                   _SPLIT_SKIPLOC disco_apply + the split kernel with the step-1 block skipped, _WHOLE disco_apply + a
 *                                   kernel that sums the whole triangle.  Options "room_cov", disco_set_tuning and disco_set_lengths
 *                                   apply as in the whole path (per-room lengths: the statistics and the room pass read nothing beyond a
 *                                   room's frames; disco_apply does, so off the room pass X must hold zeros there, as the library's own
 *                                   spectra do).  No node shard.
 *   disco_selftest_pending_matrices Rss, Rnn [R][Kl][F][P][P] of the pending pencil (it stays pending): the partial blocks combined in
 *                                   float64, scaled by 1 / T (1 / T_r under per-room lengths) and rounded once, mirrored.  A pencil pending as
 *                                   tail blocks takes the entries with both indices below M from the kept step-1 blocks, as the solvers'
 *                                   loaders do; a whole-triangle pencil gives the bits disco_cov_masked hands out. */
#define DISCO_STAGED_ROUTE_ROOM 1
#define DISCO_STAGED_ROUTE_SPLIT_SKIPLOC 2
#define DISCO_STAGED_ROUTE_WHOLE 3
int disco_selftest_staged_step2(disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* w_loc, disco_c32* z, int store_z,
                                int* route_out, disco_stream s);
int disco_selftest_pending_matrices(disco_ctx* ctx, disco_c32* Rss, disco_c32* Rnn, disco_stream s);

#define DISCO_PK_SELFTEST_OPS 23
int disco_selftest_pk(disco_ctx* ctx, const disco_c32* a, const disco_c32* b, const disco_c32* c, int64_t n,
                      disco_c32* out_hw, disco_c32* out_ref, disco_stream s);

#ifdef __cplusplus
}
#endif
#endif /* DISCO_HIP_H */
