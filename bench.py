#!/usr/bin/env python3
"""Benchmark of the MI355X MWF hot path (driver contract: ONE JSON line on rank 0).

Headline workload: `--config` picks one of BASELINE.json's configurations (default C3, the one the metric is quoted on):
  C2       256 rooms x 1 node  x 4 mics, 512-pt STFT, oracle mask            (single node: step 1 + iSTFT)
  C3       1000 rooms x 4 nodes x 4 mics, 512-pt STFT, oracle mask, z exchange on the GPU
  C4       C3's shape with CRNN masks (PyTorch-ROCm) in the loop, 125 rooms per GPU (1000 rooms over 8 GPUs)
  C5       200 rooms x 8 nodes x 8 mics, 1024-pt STFT, 2 step-2 iterations (DANSE-style stress shape)
all at 16 kHz, 10 s clips (L = 160000); --rooms/--nodes/--mics/--n-fft/--iters/--mask override single fields.
One "step" = the whole path over the whole batch: oracle mask (2 STFTs/node) -> STFT -> covariance -> GEVD-MWF solve -> z ->
exchange -> covariance -> solve -> filter -> iSTFT, inputs and outputs resident in HBM.  metric = node-frames/s (1 node-frame =
one hop of all M mics of one node); x real-time = audio seconds per room / seconds per step.

The plain command (`python bench.py [--gpus N] [--steps K] [--warmup W]`) does only what the headline figure needs: it sets up,
warms up, times the steps, writes --dump-outputs and prints the line (`roofline`, `cpu_baseline` and `parity_sample` absent or null).
`--full` adds, after the headline's timed region: the sampled-room oracle check, the per-stage timing pass behind `roofline` and
`stages`, the CPU baseline and -- for the plain C3 headline -- the other BASELINE configurations for a few steps each (C5, C2 at 256
and 4000 rooms, C4 and the online mode), attached as `"configs": {name: {ms_per_step, value, roofline, parity_sample, stages, ...}}`
(`--extras none` skips them, `--extras C5,C2` picks).  The headline fields are untouched by any of it.

Multi-GPU (`--gpus N`): one process per GPU.  Under torch.distributed.run (RANK/WORLD_SIZE in the environment) the ranks are
taken as given; started plainly with --gpus N > 1 the script launches its own N ranks (disco_amd/dist.py:launch_ranks).
  --shard rooms (default): rooms shard across ranks with NO data-path collective (weak scaling: `--rooms` per GPU); RCCL only
                           carries the timing barrier / max / sum of the contract.
  --shard nodes          : the nodes of every room are split over the ranks and z is exchanged with one RCCL all-gather per
                           step-2 iteration -- the exchange DISCO's algorithm performs (tango.py:378-386); the line then carries
                           the all-gather's bytes per rank and link rate.
With --full, EVERY rank checks sampled rooms of ITS OWN batch -- the output of the last timed step -- against the float64 CPU oracle
("parity_sample": rank 0's rooms in `per_room`, every rank's rooms / device / worst error in `ranks`, the worst over all
ranks in `worst_rel_all_ranks`); a failure on any rank exits non-zero after the line is printed.  The oracle runs in worker
processes while the GPU goes on with the next workload.
`--dump-outputs DIR` writes what the headline's last timed step computed (rank 0's enhanced signals and masks, float32 .npy, a fixed
seeded sample of rooms within DUMP_BYTES); every input is generated from fixed seeds, so two builds run with the same arguments can be
compared output for output.
"""
import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# Parity bar of every workload: 1e-4 (BASELINE.json north_star), two-step and iterated alike.  (Round 3 held the DANSE-style ITERATED
# scheme, C5, to 3e-4: its float32 sums over 157 frames left room 199 at 2.3e-4.  Round 4 shortened the sums -- time sub-chunks across
# the lanes of the room pass, float64 step-1 statistics -- and the relaxed bar is gone.)
PARITY_TOL = 1.0e-4
DUMP_BYTES = 60 << 20      # --dump-outputs: every array together, float32 (the .npy headers stay well inside the 64 MB cap)
HBM_ACHIEVABLE = 6.3e12    # /opt/skills/guides/MI355X_MICROARCH.md: what a streaming kernel reaches; a stage "moving" more than that has a wrong byte model
HBM_PEAK = 8.0e12          # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s measured achievable)
BF16_MATRIX_PEAK = 2.5e15   # same guide: dense bf16 MFMA peak (the headline figures with 2:1 sparsity are never used)
F32_MATRIX_PEAK = 157.3e12  # same guide: f32-input MFMA = the f32 vector rate (what a float32 library GEMM / convolution can reach)

CONFIGS = {
    'C2': dict(rooms=256, nodes=1, mics=4, n_fft=512, iters=1, mask='oracle', online_every=0),
    'C3': dict(rooms=1000, nodes=4, mics=4, n_fft=512, iters=1, mask='oracle', online_every=0),
    'C4': dict(rooms=125, nodes=4, mics=4, n_fft=512, iters=1, mask='crnn', online_every=0),
    'C5': dict(rooms=200, nodes=8, mics=8, n_fft=1024, iters=2, mask='oracle', online_every=0),
}
# what --full runs after the plain C3 headline (name -> workload, steps, warmup, rooms rank 0 checks against the oracle)
EXTRAS = {
    # (the launch-bound C2 first, right behind the headline: a 0.9 ms step does not survive the host being shared with the oracle
    # workers of a wide-shape workload -- 2.8 instead of 0.87 ms behind C5's three 8 x 8 rooms)
    'C2': (dict(CONFIGS['C2'], also_graph=True), 30, 3, 4),
    'C2x4000': (dict(CONFIGS['C2'], rooms=4000), 5, 2, 4),
    'online1': (dict(CONFIGS['C3'], online_every=1), 2, 1, 3),
    'C5': (dict(CONFIGS['C5']), 5, 2, 8),       # round 5: 8 of the 200 rooms (an 8 x 8 room costs the oracle ~11 s on one core)
    'C4': (dict(CONFIGS['C4']), 3, 1, 32),      # 32 of the 125 rooms (a 4 x 4 room costs the oracle ~1 s; rooms with saturated bins also run the reference-dtype oracle: score_given_masks)
    'C4_bf16': (dict(CONFIGS['C4'], dnn_dtype='bf16'), 3, 1, 2),      # the networks' convolutions / GEMMs on bf16 operands (explicit switch)
}


def b_alg(M, K, F, H, iters=1):
    """algorithmic bytes per node-frame of the whole path ('enhanced' outputs)."""
    if K == 1:
        return 8 * M * H + 4 * F + 4 * H
    base = 16 * M * H + 8 * F + 16 * (K - 1) * F + 8 * F + 4 * H
    return base + (iters - 1) * (8 * M * H + 4 * F + 16 * (K - 1) * F + 8 * F)


def kernel_alg_bytes(M, K, F, H):
    """Compulsory bytes per node-frame of each stage given its C-ABI contract (inputs once + outputs once);
    DESIGN.md section 'Kernels' derives them.  Keys are the library's stage names (disco_stage_report)."""
    return {
        'mask_oracle': 2 * H * 4 + F * 4,                     # s_ref, n_ref hop samples in, mask out
        'stft': M * H * 4 + M * F * 8,                        # hop samples of M mics in, M*F bins out
        'stft_cov1': M * H * 4 + M * F * 8 + F * 4,           # samples + mask in, X out (covariances amortised over T)
        'stft_cov1_nostore': M * H * 4 + F * 4,               # samples + mask in (X not materialised)
        'cov1': M * F * 8 + F * 4,                            # X + mask in (covariances: amortised over T)
        'apply1': M * F * 8 + F * 8,                          # X in, z out
        'cov2': M * F * 8 + F * 4 + (K - 1) * F * 8,          # X + mask + remote z in
        'room_cov2': M * F * 8 + F * 4 + F * 8,               # X + mask in, z out (all nodes of a room in one workgroup: remote z's stay on chip)
        'apply2': M * F * 8 + F * 8 + F * 8,                  # X + z in (every z row once per room: the K - 1 readers of a row share it on chip / in L2), yf out
        'step2_cov': M * F * 8 + F * 4,                       # X + mask in (z stays on chip)
        'step2_apply': M * F * 8 + F * 8,                     # X in, yf out
        'step2_apply_istft': M * F * 8 + H * 4,               # X in, hop samples out (yf stays on chip)
        'stft_apply_istft': M * H * 4 + H * 4,                # samples in, hop samples out (single node, nothing materialised)
        'istft': F * 8 + H * 4,                               # yf in, hop samples out
        'apply2_istft': M * F * 8 + F * 8 + H * 4,            # X + z in, hop samples out (wide shapes: yf stays on chip)
        'apply_istft': M * F * 8 + H * 4,
        'online1': M * F * 8 + F * 4 + F * 8,                 # X + mask in, z out (the smoothed matrices live in registers)
        'online2': M * F * 8 + (K - 1) * F * 8 + F * 4 + F * 8,   # X + remote z + mask in, yf out
    }


def csrc_digest():
    """Identity of the kernel sources a PMC traffic file was measured on (profiles/pmc_traffic*.json carry it)."""
    h = hashlib.sha256()
    d = os.path.join(REPO, 'disco_amd', 'csrc')
    for f in sorted(os.listdir(d)):
        h.update(f.encode())
        h.update(open(os.path.join(d, f), 'rb').read())
    return h.hexdigest()[:16]


_WORKER = r"""
import sys, time
sys.path.insert(0, sys.argv[1])
room, K, M, L, start_at, n_fft = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]), int(sys.argv[7])
from disco_amd import synth
from oracle import tango_oracle as to
y, s, n, _ = synth.make_room_numpy(room, K=K, M=M, L=L)
late = time.time() > start_at
while time.time() < start_at:
    time.sleep(0.005)
t0 = time.time()
to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], n_fft=n_fft, hop=n_fft // 2, precision='f64', solver='eigh')
print(t0, time.time(), int(late))
"""


def cpu_vectorised_all_cores(K, M, L, n_fft=512, lead_seconds=20.0, limit_seconds=90.0):
    """the vectorised oracle on every host core at once -- one single-threaded process per core, one room
    each, all released at the same wall-clock instant; rate = rooms done / (last finish - common start).  Plain
    subprocesses with a hard time limit: a reported baseline must never be able to hang or fail the bench."""
    import subprocess
    procs = os.cpu_count() or 1
    env = dict(os.environ, OMP_NUM_THREADS='1', OPENBLAS_NUM_THREADS='1', MKL_NUM_THREADS='1')
    start_at = time.time() + lead_seconds
    ps = []
    try:
        for r in range(procs):
            ps.append(subprocess.Popen([sys.executable, '-c', _WORKER, REPO, str(r), str(K), str(M), str(L), repr(start_at), str(n_fft)],
                                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, text=True))
        ends, late = [], 0
        for p in ps:
            out, _ = p.communicate(timeout=max(1.0, start_at + limit_seconds - time.time()))
            t0, t1, lt = out.split()
            ends.append(float(t1))
            late += int(lt)
        if late:
            return {'error': f'{late} of {procs} workers were not ready at the common start'}
        wall = max(ends) - start_at
    except Exception as e:
        for p in ps:
            if p.poll() is None:
                p.kill()
        return {'error': repr(e)}
    T = 1 + L // (n_fft // 2)
    return {'value': procs * K * T / wall, 'unit': 'node-frames/s', 'cores': procs, 'seconds': round(wall, 2),
            'what': f'{procs} processes x 1 room each (OMP_NUM_THREADS=1), released together, '
                    'oracle/tango_oracle.py:offline_tango_vec'}


def cpu_baseline(K, M, L, n_fft=512):
    """The reference's CPU path (literal loop nest, oracle/tango_oracle.py:offline_tango_literal -- pinned bit-exact against
    the reference's own code) on a bounded sample of the same workload, one host core: one room when that fits ~30 s, else
    the first nodes' worth the clock allows (the literal loop nest costs ~2 s per node at 4 mics, ~8x that at 8 mics / P = 15)."""
    from disco_amd import synth
    from oracle import tango_oracle as to
    hop = n_fft // 2
    Ls = L if K * M <= 16 else L // 8                     # C5-shaped rooms: an eighth of the clip keeps the sample bounded
    y, s, n, _ = synth.make_room_numpy(0, K=K, M=M, L=Ls)
    Ts = 1 + Ls // hop
    t0 = time.perf_counter()
    to.offline_tango_literal(y, s, n, vads=['irm1', 'irm1'], n_fft=n_fft, hop=hop)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], n_fft=n_fft, hop=hop, precision='f64', solver='eigh')
    dtv = time.perf_counter() - t0
    return {'value': K * Ts / dt, 'unit': 'node-frames/s', 'cores': 1, 'kind': 'port',
            'vectorised_numpy': {'value': K * Ts / dtv, 'unit': 'node-frames/s', 'seconds': round(dtv, 2),
                                 'what': 'oracle/tango_oracle.py:offline_tango_vec (float64, einsum covariances, batched eigh), same sample'},
            'vectorised_numpy_all_cores': cpu_vectorised_all_cores(K, M, L, n_fft) if K * M <= 16 else None,
            'sample': f'1 room ({K} nodes x {M} mics, {Ls} of {L} samples = {K * Ts} node-frames), literal reference loop nest '
                      f'(tango.py:326-457 restated, bit-exact vs reference), STFTs included, {dt:.1f} s on 1 of '
                      f'{os.cpu_count()} host cores',
            'x_realtime': (Ls / 16000.0) / dt}


# ---- the checker: sampled rooms against the float64 CPU oracle (runs in worker processes) ------------------------------------------
def parity_job_file(path):
    """parity_job on a room parked in an .npz file (written synchronously by the bench process BEFORE it goes on: handing the arrays
    -- 40 MB for a C5 room -- to the worker through the executor's pickling thread would hold the interpreter lock of the bench
    process at an arbitrary later moment, e.g. inside the next workload's timed region).  The file is removed."""
    import numpy as np
    with np.load(path, allow_pickle=False) as d:
        masks = None
        if 'mz' in d.files:
            masks = ([m for m in d['mz']], [m for m in d['mw']])
        yf_hip = d['yf_hip'] if 'yf_hip' in d.files else None
        args = (str(d['kind']), int(d['room']), d['yr'], d['sr'], d['nr'], d['got'], int(d['k0']), int(d['n_fft']), int(d['iters']), masks, yf_hip)
    os.remove(path)
    return parity_job(*args)


def parity_job(kind, room, yr, sr, nr, got, k0, n_fft, iters, masks=None, yf_hip=None):
    """One sampled room of the batch the timed region just processed, against the float64 CPU oracle (test infrastructure used as
    the checker, never as the thing measured).  yr (K,M,L); sr, nr (K,L) target / noise image at the reference mic; got (Kl,L):
    this rank's nodes [k0, k0+Kl) of the room's output.  kind: 'batch' (offline_tango_vec, oracle masks), 'masks' (the same
    around GIVEN masks: the DNN's predictions go to both sides; yf_hip (K,T,F): the filtered spectra of the timed step, see
    score_given_masks), 'online' (online_oracle.online_tango).  -> (room, worst rel err[, info dict])."""
    import numpy as np
    from oracle import stft_oracle as so
    L = yr.shape[-1]
    s = np.zeros_like(yr)
    n = np.zeros_like(yr)
    s[:, 0] = sr                                          # the masks only look at the reference microphone (tango.py:338-342)
    n[:, 0] = nr
    if kind == 'masks':
        e, info = score_given_masks(yr, s, n, got, masks, yf_hip, n_fft, seed=int(room))
        return int(room), e, info
    if kind == 'online':
        from oracle import online_oracle as oo
        ref_out = oo.online_tango(yr, s, n, n_fft=n_fft, hop=n_fft // 2, update_every=iters)['out']
        refs = [ref_out[k0 + kl] for kl in range(got.shape[0])]
    else:
        from oracle import tango_oracle as to
        o = to.offline_tango_vec(yr, s, n, n_fft=n_fft, hop=n_fft // 2, precision='f64', solver='eigh', vads=['irm1', 'irm1'], extra_iters=iters - 1)
        refs = [so.istft(o['yf'][k0 + kl], L, n_fft, n_fft // 2, work_dtype=np.float64) for kl in range(got.shape[0])]
    e = 0.0
    for kl in range(got.shape[0]):
        e = max(e, float(np.linalg.norm(got[kl] - refs[kl]) / np.linalg.norm(refs[kl])))
    return int(room), e


# ---- PREDICTED masks (C4): every sampled room, every bin is asserted (round-5 VERDICT: no room is set aside) ------------------------------
# A pencil (Rss, Rnn) of a bin is built from the frames weighted m^2 and (1 - m)^2 (tango.py:357-364, 433-440).  Predicted masks that saturate
# over most frames of a bin leave a statistic with next to no weight, or with its weight on fewer frames than the pencil has rows: a pencil whose
# dominant generalized eigenvector float32 inputs do not determine to 1e-4, whoever solves it.  The float64 Cholesky / eigh oracle is not the
# yardstick there; what DEFINES the behaviour is the reference's own arithmetic -- complex64 statistics, scipy.linalg.eig + the eps / 1e6 clamps
# (internal_formulas.py:56-73), restated bit-exactly by oracle/mwf_oracle.py:intern_filter (precision 'ref32', solver 'eig').  Bins are independent
# from the STFT to the iSTFT, over both steps and all nodes of a room (the exchanged z of bin f only enters bin f), so a room is scored per bin:
#   flagged bins B: the float64 oracle's own output in the bin moves by more than tol / 20 when its inputs move by what float32 cannot resolve
#       -- every mask value by one float32 rounding, every sample by 3e-7 (the accuracy class of a float32 512-point transform); two random sign
#       patterns, the larger movement counts -- or a (step, node) statistic of the bin has less than FLAG_WEIGHT frames of weight.  Measured on
#       C4's random-weight masks: 80 - 220 of a room's 257 bins (tools/gpu/exp_c4_perbin.py, profiles/r06_d_c4_perbin_summary.txt).
#   (a) the other bins, per node: || yf_hip - yf_f64 || over them / || yf_f64 || (the node's whole spectrum) < tol -- the 1e-4 bar on what they put into
#       the output (relative to their own energy the figure would be set by how FEW bins are left: a room with 225 of 257 bins flagged);
#   (b) the flagged bins, per node: E_hip(B) = || yf_hip - yf_f64 ||_B  <=  max(tol || yf_f64 ||, 2 E_ref32(B)): within the bar, or within twice
#       the distance the reference's OWN arithmetic keeps from the same oracle on those pencils;
#   (c) the spectra scored are those of the timed step (bench re-derives them with the same kernel sequence on the same masks): their iSTFT
#       against the timed output.
# Reported beside it, per room: the worst (node, bin) with e_hip, e_ref32 and the measured sensitivity -- the HIP path is typically 3 - 6 x the
# float32-class sensitivity of a bin (its transform is float32 where the reference rounds a float64 transform to complex64) and far inside the
# reference's own noise on the singular ones.
FLAG_WEIGHT = 1e-4            # a statistic with less than this many frames' worth of weight flags the bin (units of one frame's weight)
FLAG_SENS = 1.0 / 20          # ... as does an oracle output that moves by more than FLAG_SENS * tol under a float32-class input perturbation
F32_SAMPLE_NOISE = 3e-7       # relative accuracy class of a float32 512-point transform (measured: tests' STFT bound 2e-6 max, ~3e-7 rms)


def flagged_bins(masks):
    """The weight rule alone.  masks: (masks_z, masks_w), each a list over nodes of (F, T) arrays -> (sorted bin indices, smallest weight)."""
    import numpy as np
    bad, wmin = None, np.inf
    for ms in masks:
        for m in ms:
            m = np.asarray(m, np.float64)
            ws, wn = (m * m).sum(axis=-1), ((1.0 - m) ** 2).sum(axis=-1)
            b = (ws < FLAG_WEIGHT) | (wn < FLAG_WEIGHT)
            bad = b if bad is None else (bad | b)
            wmin = min(wmin, float(ws.min()), float(wn.min()))
    return np.flatnonzero(bad), wmin


def score_given_masks(yr, s, n, got, masks, yf_hip, n_fft, tol=PARITY_TOL, seed=0):
    """-> (figure of merit e: the room passes iff e < tol, info).  e = max over (a) the error over the unflagged bins relative to the whole spectrum, (b) tol x
    E_hip(B) / max(tol ||yf||, 2 E_ref32(B)) over the flagged bins, (c) the distance between the iSTFT of the handed-over spectra and the
    timed output -- each the worst over the nodes.  Without spectra (yf_hip None): the whole time-domain output at tol."""
    import numpy as np
    from oracle import stft_oracle as so
    from oracle import tango_oracle as to
    K, L = yr.shape[0], yr.shape[-1]
    hop = n_fft // 2

    def run(y_, masks_, precision='f64'):
        o_ = to.offline_tango_vec(y_, s, n, n_fft=n_fft, hop=hop, precision=precision, solver='eigh' if precision == 'f64' else 'eig', masks=masks_)
        return np.stack([np.asarray(o_['yf'][k]).astype(np.complex128) for k in range(K)])                    # (K, F, T)
    Yf = run(yr, masks)
    if yf_hip is None:
        e = max(float(np.linalg.norm(got[k] - so.istft(Yf[k], L, n_fft, hop, work_dtype=np.float64)) / np.linalg.norm(so.istft(Yf[k], L, n_fft, hop, work_dtype=np.float64)))
                for k in range(K))
        return e, {'flagged_bins': 0, 'note': 'no spectra handed over: the whole time-domain output at tol'}
    den = np.linalg.norm(Yf, axis=-1)                                                                         # (K, F)
    den = np.where(den > 0, den, 1.0)
    # ---- which bins float32 inputs do not determine to the bar
    fb_w, wmin = flagged_bins(masks)
    sens = np.zeros_like(den)
    rng = np.random.default_rng(1000 + seed)
    for _ in range(2):
        pert = tuple([np.clip(np.asarray(m, np.float64) * (1.0 + 6e-8 * rng.choice([-1.0, 1.0], size=np.shape(m))), 0.0, 1.0) for m in ms] for ms in masks)
        yp = yr.astype(np.float64) * (1.0 + F32_SAMPLE_NOISE * rng.choice([-1.0, 1.0], size=yr.shape))
        sens = np.maximum(sens, np.linalg.norm(run(yp, pert) - Yf, axis=-1) / den)
    flag = sens.max(axis=0) > FLAG_SENS * tol
    flag[fb_w] = True
    Yh = np.transpose(np.asarray(yf_hip), (0, 2, 1)).astype(np.complex128)
    dh = np.linalg.norm(Yh - Yf, axis=-1)                                                                     # (K, F) absolute
    nall = np.linalg.norm(Yf, axis=(1, 2))
    e_cons = max(float(np.linalg.norm(so.istft(Yh[k], L, n_fft, hop, work_dtype=np.float64) - got[k]) / np.linalg.norm(got[k])) for k in range(K))
    keep = ~flag
    e_unfl = float(max(np.linalg.norm(dh[k][keep]) / nall[k] for k in range(K))) if keep.any() else 0.0      # what the unflagged bins put into the node's whole output
    info = {'flagged_bins': int(flag.sum()), 'flagged_by_weight': int(fb_w.size), 'min_statistic_weight': wmin, 'unflagged_rel': e_unfl,
            'spectra_vs_timed_output': e_cons}
    e_fl = 0.0
    if flag.any():
        # the reference's own arithmetic on the same masks (float32 masks, complex64 statistics, scipy.linalg.eig + clamps)
        m32 = tuple([np.asarray(m, np.float32) for m in ms] for ms in masks)
        with np.errstate(all='ignore'):
            try:
                dr = np.linalg.norm(run(yr, m32, 'ref32') - Yf, axis=-1)
                dr = np.where(np.isfinite(dr), dr, np.inf)          # a bin where the reference's path returns no finite answer: no bound from it
            except Exception as ex:                                 # (LinAlgError on an exactly singular eigenvector matrix)
                dr = np.full_like(dh, np.inf)
                info['reference_dtype_run'] = repr(ex)[:80]
        Eh = np.array([np.linalg.norm(dh[k][flag]) for k in range(K)])
        Er = np.array([np.linalg.norm(dr[k][flag]) for k in range(K)])
        Es = np.array([np.linalg.norm((sens * den)[k][flag]) for k in range(K)])
        ratio = Eh / np.maximum(tol * nall, 2.0 * Er)
        e_fl = float(ratio.max())
        finite = bool(np.isfinite(Yh).all())
        if not finite:
            e_fl = float('inf')
        rel_h, rel_r = dh / den, dr / den
        score = np.where(flag[None, :], rel_h / np.maximum(np.maximum(2.0 * rel_r, 10.0 * sens), tol), 0.0)
        k_, f_ = np.unravel_index(int(np.argmax(score)), score.shape)
        info.update({'flagged_hip_over_norm': [float(x) for x in Eh / nall], 'flagged_ref32_over_norm': [float(min(x, 1e30)) for x in Er / nall],
                     'flagged_f32_sensitivity_over_norm': [float(x) for x in Es / nall], 'flagged_ratio': e_fl,
                     'flagged_without_finite_reference': int((~np.isfinite(dr[:, flag])).sum()),
                     'worst_bin': {'bin': int(f_), 'node': int(k_), 'hip_vs_f64': float(rel_h[k_, f_]), 'ref32_vs_f64': float(min(rel_r[k_, f_], 1e30)),
                                   'f32_sensitivity': float(sens[k_, f_]), 'hip_over_max_2ref32_10sens_tol': float(score[k_, f_])}})
    return max(e_unfl, e_cons, tol * e_fl), info


def rank_sample_rooms(rank, R, n_rank0):
    """Local room indices a rank checks: rank 0 spreads `n_rank0` over its batch (first ... last); every other rank takes ONE room of
    its own, at a rank-dependent position (so that a wrong room range or device on rank r shows up)."""
    if rank == 0:
        n_s = max(1, min(n_rank0, R))
        return sorted({int(round(i * (R - 1) / max(n_s - 1, 1))) for i in range(n_s)})
    return [(37 * rank + R // 2) % R]


def merge_parity(local, per_rank_rows, tol):
    """local: rank 0's {'rooms', 'per_room', 'worst_rel'}; per_rank_rows: [(rank, device, first_room, [global room ids], worst)] of
    EVERY rank -> the parity_sample object of the line."""
    worst_all = max(r[4] for r in per_rank_rows)
    return {'rooms': local['rooms'], 'worst_rel': local['worst_rel'], 'tol': tol, 'ok': bool(worst_all < tol),
            'per_room': local['per_room'], 'worst_rel_all_ranks': worst_all,
            'ranks': [{'rank': int(r[0]), 'device': int(r[1]), 'first_room': int(r[2]), 'rooms_checked': [int(x) for x in r[3]],
                       'worst_rel': r[4]} for r in per_rank_rows],
            'oracle': 'float64 CPU oracle (oracle/tango_oracle.py:offline_tango_vec + oracle/stft_oracle.py:istft; online: '
                      'oracle/online_oracle.py:online_tango), per (room, node) ||out - ref||_2 / ||ref||_2 on the output of the last '
                      'timed step; every rank checks rooms of its own batch'}


def gather_rank_rows(rank, world, device_index, first_room, rooms_global, worst, dist, dev, gloo=False):
    """All-gather of every rank's (device, first room, checked rooms, worst error) as one fixed-size float64 row."""
    import torch
    row = [float(rank), float(device_index), float(first_room), float(min(len(rooms_global), 4))] + [float(x) for x in rooms_global[:4]]
    row += [-1.0] * (8 - len(row)) + [float(worst)]
    if world == 1:
        rows = [row]
    else:
        t = torch.tensor(row, dtype=torch.float64, device='cpu' if gloo else dev)
        outs = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(outs, t)
        rows = [o.cpu().tolist() for o in outs]
    return [(int(r[0]), int(r[1]), int(r[2]), [int(x) for x in r[4:4 + int(r[3])]], float(r[8])) for r in rows]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20, help='timed steps of the headline workload (at least 1)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='after the timed steps, write what the headline\'s last timed step computed (rank 0) as DIR/<name>.npy, float32: '
                         'enhanced (rooms, nodes, length) and the masks it ran on; a fixed seeded sample of the rooms when the whole '
                         f'batch exceeds {DUMP_BYTES >> 20} MiB')
    ap.add_argument('--config', default='C3', choices=sorted(CONFIGS), help='BASELINE.json configuration (shape defaults)')
    ap.add_argument('--rooms', type=int, default=None, help='rooms per GPU')
    ap.add_argument('--nodes', type=int, default=None)
    ap.add_argument('--mics', type=int, default=None)
    ap.add_argument('--length', type=int, default=160000)
    ap.add_argument('--n-fft', type=int, default=None)
    ap.add_argument('--mask', default=None, choices=['oracle', 'crnn'],
                    help="'crnn': BASELINE configs[3] -- randomly initialised CRNN mask estimators (PyTorch-ROCm) in the loop")
    ap.add_argument('--online-every', type=int, default=None,
                    help='> 0: time the ONLINE pipeline (SURVEY 8f-2) with a filter update every this many frames instead of '
                         'the batch path (not the headline metric)')
    ap.add_argument('--iters', type=int, default=None,
                    help='> 1: the DANSE-style iterated scheme (BASELINE configs[4]; disco_tango_enhance_iterated)')
    ap.add_argument('--shard', default='rooms', choices=['rooms', 'nodes'],
                    help="'nodes': split the nodes of every room over the ranks, one RCCL all-gather of z per step-2 iteration")
    ap.add_argument('--overlap-exchange', action='store_true',
                    help='--shard nodes: run the step as two half-batches whose all-gathers overlap the other half\'s kernels (opt-in: no run on '
                         '>= 2 GPUs over RCCL has been recorded); the exchange statistics then come from a separate non-overlapped pass')
    ap.add_argument('--graph', action='store_true',
                    help='capture one step (mask + whole path) into a hipGraph on a side stream and time its replays: one launch per '
                         'step instead of 6-20 (matters for small batches; oracle masks, room-sharded batch path only)')
    ap.add_argument('--full', action='store_true',
                    help='also run what the headline figure does not need: the sampled-room oracle check, the per-stage timing pass '
                         '(roofline, stages; the online stream), the CPU baseline and the other BASELINE configurations (--extras). '
                         'Without it the command sets up, warms up, times the steps, writes --dump-outputs and prints the line')
    ap.add_argument('--extras', default='auto',
                    help="--full: the other BASELINE configurations run after the headline and attached as `configs`: 'auto' (all of "
                         f"{', '.join(EXTRAS)} when the command is the plain C3 headline, none otherwise), 'all', 'none', or a comma list")
    ap.add_argument('--tuning', default=None, help='disco_set_tuning values a,b,c,d for the headline workload (experiments)')
    ap.add_argument('--detail', default=None, help='where the full result goes (default: bench_detail.json at the repo root, and gpurun_out/ when present); stdout carries the compact line')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without the CPU baseline')
    ap.add_argument('--no-stage-timing', action='store_true', help='--full without the per-stage timing pass')
    ap.add_argument('--no-parity', action='store_true', help='--full without the sampled-room oracle check after the timed region')
    ap.add_argument('--parity-rooms', type=int, default=6)
    ap.add_argument('--parity-workers', type=int, default=8, help='oracle worker processes per rank (sweeps of whole batches: raise it on a many-core host)')
    ap.add_argument('--pmc-calibrate', action='store_true', help='also run a 4 GiB device copy (known bytes) for PMC calibration')
    ap.add_argument('--dist-backend', default='nccl', choices=['nccl', 'gloo'],
                    help="'gloo' + --single-device: a functional test of the N > 1 bookkeeping on a box with ONE GPU (every rank computes on cuda:0, "
                         'the control collectives go over gloo); not a measurement')
    ap.add_argument('--single-device', action='store_true', help='every rank uses cuda:0 (test only, see --dist-backend)')
    ap.add_argument('--dry-collective', action='store_true',
                    help='no GPU work (--shard nodes): every rank joins a gloo group and runs the z exchange of the node-sharded step -- the same '
                         'all_gather_into_tensor calls on CPU tensors of the real per-rank size, content checked -- and rank 0 prints the line\'s '
                         '`exchange` object (bytes per rank / per peer link, ms per gather).  Bookkeeping of the N > 1 path on a box without GPUs; not a measurement')
    ap.add_argument('--selftest-launch', action='store_true',
                    help='no GPU work: every rank joins a gloo group, rank 0 prints n_gpus and the all-rank parity merge of fake per-rank '
                         'errors (covers the self-launch path and the all-rank bookkeeping on CPU)')
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error('--steps: at least one timed step')
    cfg = CONFIGS[args.config]
    plain = all(getattr(args, k) is None for k in ('rooms', 'nodes', 'mics', 'n_fft', 'iters', 'mask', 'online_every'))
    for k in ('rooms', 'nodes', 'mics', 'n_fft', 'iters', 'mask', 'online_every'):
        if getattr(args, k) is None:
            setattr(args, k, cfg[k])
    if not args.full:
        if args.extras not in ('auto', 'none'):
            ap.error('--extras: the other configurations run with --full')
        args.extras = 'none'
        args.no_cpu_baseline = args.no_stage_timing = args.no_parity = True
    if args.extras == 'auto':
        args.extras = 'all' if (plain and args.config == 'C3' and args.shard == 'rooms' and not args.graph and args.length == 160000) else 'none'
    if args.extras == 'all':
        args.extra_names = [n for n in EXTRAS if n != 'C4_bf16']       # the bf16 variant on request only (--extras C4,C4_bf16)
    elif args.extras == 'none':
        args.extra_names = []
    else:
        args.extra_names = [x for x in args.extras.split(',') if x]
        bad = [x for x in args.extra_names if x not in EXTRAS]
        if bad:
            ap.error(f'--extras: unknown workload(s) {bad}; known: {list(EXTRAS)}')
    return args


class TorchStageMarks:
    """Phase timer of the PyTorch-driven path (C4): an event on the launch stream after every phase."""

    def __init__(self, torch):
        self.torch = torch
        self.ev = []
        self('start')

    def __call__(self, name):
        e = self.torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append((name, e))

    def report(self, rooms):
        self.torch.cuda.synchronize()
        out = {}
        for (_, a), (name, b) in zip(self.ev[:-1], self.ev[1:]):
            ms, n, r = out.get(name, (0.0, 0, 0))
            out[name] = (ms + a.elapsed_time(b), n + 1, r + rooms)
        return out


def run_workload(name, w, steps, warmup, env, headline, n_parity_rank0, args):
    """Generate the synthetic batch of workload `w` on this rank's GPU, time `steps` steps, time the stages, hand sampled rooms of
    the last timed step to the oracle workers.  Collectives (barrier / max / sum) only for the headline; the extras time every
    rank on its own clock and are merged at the end (no collective inside something that may fail on one rank only).
    -> (result dict, parity ticket)"""
    import numpy as np
    import torch
    from disco_amd import dist as dd
    from disco_amd import synth
    from disco_amd.engine import Engine

    rank, world, local_rank, dev, dist, lib = env['rank'], env['world'], env['local_rank'], env['dev'], env['dist'], env['lib']
    R, K, M, Ls, N = w['rooms'], w['nodes'], w['mics'], args.length, w['n_fft']
    iters, mask_kind, online_every = w['iters'], w['mask'], w['online_every']
    H, F = N // 2, N // 2 + 1
    node_sharded = headline and args.shard == 'nodes'
    if node_sharded and (mask_kind != 'oracle' or online_every):
        raise SystemExit('--shard nodes runs the batch path with oracle masks')
    eng = Engine(rooms=R, nodes=K, mics=M, length=Ls, n_fft=N, device=local_rank, lib=lib)
    T = eng.T
    if headline and args.tuning:
        eng.set_tuning(*[int(x) for x in args.tuning.split(',')])
    assert torch.cuda.current_stream().cuda_stream == 0, 'bench times the null stream the library launches on'

    want_parity = not args.no_parity
    sample_rooms = rank_sample_rooms(rank, R, n_parity_rank0) if want_parity else []
    sample_in = {}

    # synthetic rooms, generated on the GPU (SURVEY 8d recipe)
    if node_sharded:
        from disco_amd import node_sharded as ns
        k0, Kl = ns.node_range(rank, world, K)
        eng.set_node_shard(k0, Kl)
        first_room = 0
        # every rank draws the same R rooms and keeps its own nodes (the generator is per room; slicing keeps it simple)
        y_all, s_all, n_all = synth.make_rooms_torch(R, K, M, Ls, first_room=0, device=dev, ref_only_sn=True)
        y = y_all[:, k0:k0 + Kl].contiguous()
        s_ref = s_all[:, k0:k0 + Kl].contiguous()
        n_ref = n_all[:, k0:k0 + Kl].contiguous()
        # the oracle needs ALL nodes of a sampled room
        sample_in = {r: (y_all[r].cpu().numpy(), s_all[r].cpu().numpy(), n_all[r].cpu().numpy()) for r in sample_rooms}
        del y_all, s_all, n_all
        units_per_step = R * Kl * T
    else:
        k0, Kl = 0, K
        first_room, _ = dd.room_range(rank, world, R)     # rank r owns rooms [r*R, (r+1)*R)
        y, s_ref, n_ref = synth.make_rooms_torch(R, K, M, Ls, first_room=first_room, device=dev, ref_only_sn=True)
        sample_in = {r: (y[r].cpu().numpy(), s_ref[r].cpu().numpy(), n_ref[r].cpu().numpy()) for r in sample_rooms}
        units_per_step = R * K * T
    mask = torch.empty((R, Kl, T, F), dtype=torch.float32, device=dev)
    out = torch.empty((R, Kl, Ls), dtype=torch.float32, device=dev)
    ws = None if node_sharded else torch.empty(eng.workspace_bytes(), dtype=torch.uint8, device=dev)
    G = R * Kl

    dnn = {}
    dnn_dtype = None
    if mask_kind == 'crnn':
        dnn_dtype = torch.bfloat16 if w.get('dnn_dtype') == 'bf16' else None
        from disco_amd.dnn.crnn import build_crnn
        from disco_amd.dnn.inloop import tango_enhance_dnn
        torch.manual_seed(0)
        model_z = build_crnn(1, device=dev)
        model_w = build_crnn(K, device=dev) if K > 1 else None
        # random weights leave every mask within a few percent of 0.5, i.e. Rss ~ Rnn in every bin: a degenerate eigenproblem whose
        # dominant vector no two implementations agree on.  Spreading the output layer (as tests/test_gpu_crnn_inloop.py does) gives
        # masks over (0, 1) like a trained network's, at identical cost.
        clip = float(os.environ.get('DISCO_BENCH_CRNN_CLIP', 0.0))
        with torch.no_grad():
            for mdl in (model_z, model_w):
                if mdl is not None:
                    mdl.ff.layers[0].weight.mul_(float(os.environ.get('DISCO_BENCH_CRNN_SPREAD', 40.0)))
                    if clip > 0:
                        mdl.predict_masks = (lambda orig: lambda *a_, **k_: orig(*a_, **k_).clamp_(clip, 1.0 - clip))(mdl.predict_masks)

    gather_events = []                     # (start, stop) torch events around every all-gather of z (--shard nodes)

    def step(mark=None):
        if mask_kind == 'crnn':
            o, mz, mw = tango_enhance_dnn(eng, y, model_z, model_w, want_masks=True, mark=mark, compute_dtype=dnn_dtype)
            out.copy_(o)
            dnn['mz'], dnn['mw'] = mz, mw
            return
        eng._chk(lib.disco_mask_oracle(eng.ctx, s_ref.data_ptr(), n_ref.data_ptr(), G, mask.data_ptr(), None))
        if node_sharded:
            ns.tango_enhance_node_sharded_torch(eng, y, mask, mask, iters=iters, out=out, want_yf=False, overlap=args.overlap_exchange,
                                                gather_events=None if args.overlap_exchange else gather_events)
            return
        if online_every > 0:
            eng._chk(lib.disco_tango_online(eng.ctx, y.data_ptr(), mask.data_ptr(), mask.data_ptr(), 0.95, online_every,
                                            1e-3, out.data_ptr(), None, None, ws.data_ptr(), ws.numel(), None))
            return
        if iters > 1:
            eng._chk(lib.disco_tango_enhance_iterated(eng.ctx, y.data_ptr(), mask.data_ptr(), mask.data_ptr(), iters,
                                                      out.data_ptr(), None, None, ws.data_ptr(), ws.numel(), None))
            return
        eng._chk(lib.disco_tango_enhance(eng.ctx, y.data_ptr(), mask.data_ptr(), mask.data_ptr(), out.data_ptr(),
                                         None, None, ws.data_ptr(), ws.numel(), None))

    def barrier():
        if world > 1 and headline:
            dist.barrier()
        torch.cuda.synchronize()

    eager_step = step

    def capture_graph():
        """The whole step (mask + path: a fixed launch sequence once the context has reserved its blocks) as ONE hipGraph -> its replay."""
        if mask_kind != 'oracle' or node_sharded or online_every:
            raise SystemExit('a graph captures the room-sharded batch path with oracle masks')
        eng.reserve(0)
        eager_step()                        # nothing is left to allocate inside the captured calls
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        hip_graph = torch.cuda.CUDAGraph()
        h = side.cuda_stream
        with torch.cuda.graph(hip_graph, stream=side):
            eng._chk(lib.disco_mask_oracle(eng.ctx, s_ref.data_ptr(), n_ref.data_ptr(), G, mask.data_ptr(), h))
            if iters > 1:
                eng._chk(lib.disco_tango_enhance_iterated(eng.ctx, y.data_ptr(), mask.data_ptr(), mask.data_ptr(), iters,
                                                          out.data_ptr(), None, None, ws.data_ptr(), ws.numel(), h))
            else:
                eng._chk(lib.disco_tango_enhance(eng.ctx, y.data_ptr(), mask.data_ptr(), mask.data_ptr(), out.data_ptr(),
                                                 None, None, ws.data_ptr(), ws.numel(), h))
        torch.cuda.synchronize()
        return hip_graph.replay             # replays on the current (null) stream, the one the barriers drain

    if args.graph and headline:
        step = capture_graph()

    if args.pmc_calibrate and headline:
        src = torch.empty(1 << 30, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        torch.neg(src, out=dst)             # 4 GiB read + 4 GiB written by ONE elementwise kernel (a plain copy_ goes to the DMA engines)
        # the same bytes with ONE dword per lane and load (the access width of the STFT kernels' sample reads): copy, then read-only
        eng._chk(lib.disco_selftest_stream(eng.ctx, src.data_ptr(), dst.data_ptr(), src.numel(), 1, None))
        eng._chk(lib.disco_selftest_stream(eng.ctx, src.data_ptr(), dst.data_ptr(), src.numel(), 0, None))
        torch.cuda.synchronize()
        del src, dst
    for _ in range(warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    barrier()
    dt_local = time.perf_counter() - t0
    if headline and args.dump_outputs and rank == 0:
        # before anything below runs the path again: these are the buffers of the last timed step
        got = {'enhanced': out}
        if mask_kind == 'crnn':
            got.update(mask_z=dnn['mz'], mask_w=dnn['mw'])
        else:
            got['mask'] = mask
        rooms = dump_outputs(args.dump_outputs, got)
        print(f'--dump-outputs: {sorted(got)} of {len(rooms)} of {R} rooms -> {args.dump_outputs}', file=sys.stderr)
    if headline:
        value, dt = dd.whole_job_throughput(units_per_step * steps, dt_local, world, device=env['cdev'])
    else:
        value, dt = units_per_step * steps / dt_local, dt_local       # merged over the ranks at the end (merge_extras)
    graph_res = None
    if w.get('also_graph') and not (args.graph and headline):
        # launch-bound small batches (C2 at 256 rooms: four launches of 0.05-0.35 ms): the same step as one hipGraph replay, reported BESIDE
        # the eager figure (which stays the workload's ms_per_step)
        try:
            replay = capture_graph()
            for _ in range(warmup):
                replay()
            torch.cuda.synchronize()
            tg = time.perf_counter()
            for _ in range(steps):
                replay()
            torch.cuda.synchronize()
            dtg = (time.perf_counter() - tg) / steps
            graph_res = {'launch': 'one hipGraph replay per step', 'ms_per_step': round(1e3 * dtg, 4), 'x_realtime': round((Ls / 16000.0) / dtg, 1),
                         'value': units_per_step / dtg,
                         'pipeline_frac': round(units_per_step / dtg * b_alg(M, K, F, H, iters) / HBM_PEAK, 4)}
            del replay
        except Exception as e:
            graph_res = {'error': repr(e)}
    finite = bool(torch.isfinite(out).all())
    if node_sharded and args.overlap_exchange:
        # an event pair around an OVERLAPPED gather also spans the other half-batch's kernels (round-5 ADVICE): the exchange is timed in its
        # own pass after the timed region, whole batch per gather, nothing beside it (--full)
        if args.full:
            for _ in range(min(steps, 3)):
                eng._chk(lib.disco_mask_oracle(eng.ctx, s_ref.data_ptr(), n_ref.data_ptr(), G, mask.data_ptr(), None))
                ns.tango_enhance_node_sharded_torch(eng, y, mask, mask, iters=iters, out=out, want_yf=False, overlap=False, gather_events=gather_events)
            torch.cuda.synchronize()
        gather_ms = [a_.elapsed_time(b_) for a_, b_ in gather_events]
    else:
        gather_ms = [a_.elapsed_time(b_) for a_, b_ in gather_events[-steps * iters:]] if gather_events else []
    ms_per_step = 1e3 * dt / steps
    x_rt = (Ls / 16000.0) / (dt / steps)

    if mask_kind == 'crnn' and want_parity and K > 1:
        # the filtered spectra of the LAST timed step (its one-pass filter + iSTFT keeps them on chip): the same kernel sequence on the same
        # masks, the final filter writing yf -- score_given_masks checks their iSTFT against the timed output
        dnn['yf'] = tango_enhance_dnn(eng, y, model_z, model_w, masks=(dnn['mz'], dnn['mw']), want_yf=True)[-1]
    # ---- sampled rooms of the last timed step -> the oracle workers (every rank, its own rooms)
    ticket = {'name': name, 'jobs': [], 'rooms_global': [first_room + r for r in sample_rooms], 'first_room': first_room,
              'tol': PARITY_TOL, 'finite': finite}
    if want_parity:
        pool = env['pool']
        for r in sample_rooms:
            yr, sr, nr = sample_in[r]
            got = out[r].cpu().numpy()
            rec = dict(room=first_room + r, yr=yr, sr=sr, nr=nr, got=got, k0=k0, n_fft=N)
            if mask_kind == 'crnn':
                rec.update(kind='masks', iters=1, mz=np.stack([dnn['mz'][r, k].T.double().cpu().numpy() for k in range(K)]),
                           mw=np.stack([dnn['mw'][r, k].T.double().cpu().numpy() for k in range(K)]))
                if dnn.get('yf') is not None:
                    rec['yf_hip'] = dnn['yf'][r].cpu().numpy()
            elif online_every > 0:
                rec.update(kind='online', iters=online_every)
            else:
                rec.update(kind='batch', iters=iters)
            path = os.path.join(env['tmpdir'], f'parity_{name}_{rank}_{first_room + r}.npz')
            np.savez(path, **rec)
            ticket['jobs'].append(pool.submit(parity_job_file, path))

    # ---- per-stage timing on the launch stream, for the roofline object (rank 0)
    roofline, stages = None, None
    if rank == 0 and not args.no_stage_timing and not node_sharded:
        reps = max(2, min(steps, 5 if headline else 3))
        # The timed region above runs the library's default: on the fused route, two half-batches on two streams (option
        # "overlap_solves").  Overlapped kernels share the chip, so an event pair around one of them measures the mix, not the kernel;
        # the per-kernel figures -- the roofline object -- are therefore taken with the option OFF: every kernel alone on the chip, the
        # whole batch per launch.  `pipeline` (whole path, timed region) is what the overlap improves.
        overlap_was = eng.get_option('overlap_solves')
        eng.set_option('overlap_solves', 0)
        eager_step()                            # the event objects are created inside the library: warm that path once
        torch.cuda.synchronize()
        # one report per step, and the MEDIAN over the steps: an event pair also spans whatever the host does between the two
        # records, and a single descheduled launch call (seen once: 85 ms inside one 7 ms stage) would otherwise own the mean
        per_rep = []
        for _ in range(reps):
            if mask_kind == 'crnn':
                marks = TorchStageMarks(torch)
                eager_step(marks)
                per_rep.append(marks.report(R))
            else:
                eng.stage_timing(True)
                eager_step()                    # (a captured graph carries no events: the stage pass always launches eagerly)
                per_rep.append(eng.stage_report())
        if mask_kind != 'crnn':
            eng.stage_timing(False)
        eng.set_option('overlap_solves', overlap_was)
        kab = kernel_alg_bytes(M, K, F, H)
        stages = {}
        for nm in per_rep[0]:
            ms_list = sorted(r_[nm][0] for r_ in per_rep if nm in r_)
            per_step = ms_list[len(ms_list) // 2] if len(ms_list) % 2 else 0.5 * (ms_list[len(ms_list) // 2 - 1] + ms_list[len(ms_list) // 2])
            launches, rooms_done = per_rep[0][nm][1], per_rep[0][nm][2]
            # rooms_done: rooms processed by all launches of the stage in one step (an iterated stage runs twice over the batch, an
            # overlapped call launches every stage once per half-batch)
            ent = {'ms': round(per_step, 4), 'launches_per_step': float(launches), 'rooms_per_step': int(rooms_done),
                   'ms_min': round(ms_list[0], 4), 'ms_max': round(ms_list[-1], 4)}
            if nm in kab:
                ent['alg_bytes'] = kab[nm] * rooms_done * K * T        # per step (all launches of the stage)
                if nm == 'room_cov2':
                    if iters > 1:
                        # only the LAST pass of an iterated run stores z (nobody reads an earlier one): 8 F per node-frame once per step
                        ent['alg_bytes'] -= (rooms_done - R) * K * T * F * 8
                    # the statistics the pass hands to the solver: per (node, bin) the M (K - 1) y-z and (K - 1) K / 2 z-z entries of both matrices as
                    # a (hi, lo) pair of float4 blocks (k_room.h `finish`).  Every other stage's statistics are "amortised over T" (< 3 % of its bytes:
                    # 10 entries per bin and chunk at M = 4); here they are 84 entries x 32 B per bin against 313 frames: 11 % of the pass's bytes
                    # (round 6: counted; rounds 4-5 read them as "wasted fetch": profiles/r05_zzz_C5_pmc_traffic.json 23.7 GB per launch)
                    ent['alg_bytes'] += rooms_done * K * F * (M * (K - 1) + (K - 1) * K // 2) * 32
                ent['GBps'] = round(ent['alg_bytes'] / (per_step * 1e-3) / 1e9, 1)
            if nm in ('crnn_z', 'crnn_w'):
                from disco_amd.dnn.crnn import flops_per_frame
                ent['flops'] = flops_per_frame(1 if nm == 'crnn_z' else K) * rooms_done * K * T
                ent['TFLOPs'] = round(ent['flops'] / (per_step * 1e-3) / 1e12, 2)
            stages[nm] = ent
        # sanity of the byte models: no stage may "move" its algorithmic bytes faster than the achievable HBM rate
        sanity = [f'{nm}: {ent["GBps"]} GB/s of algorithmic bytes exceeds the achievable HBM rate ({HBM_ACHIEVABLE / 1e9:.0f} GB/s): byte model wrong'
                  for nm, ent in stages.items() if ent.get('GBps', 0.0) > HBM_ACHIEVABLE / 1e9]
        pipeline_b = b_alg(M, K, F, H, iters)
        pipeline = {'B_alg_per_node_frame': pipeline_b, 'achieved_GBps': round(units_per_step * steps / dt_local * pipeline_b / 1e9, 1),
                    'frac': round(units_per_step * steps / dt_local * pipeline_b / HBM_PEAK, 4)}
        dom = max(stages, key=lambda n_: stages[n_]['ms'])
        lps = stages[dom]['launches_per_step']
        launch_ms = stages[dom]['ms'] / lps
        if 'flops' in stages[dom]:
            # the dominant stage is the mask-estimation DNN: float32 library GEMMs (rocBLAS / hipBLASLt) and MIOpen convolutions driven
            # by PyTorch -- not a HIP kernel of this library; priced against the float32 matrix peak
            achieved = stages[dom]['flops'] / lps / (launch_ms * 1e-3)
            peak = BF16_MATRIX_PEAK if dnn_dtype is not None else F32_MATRIX_PEAK
            roofline = {'bound': 'mfma', 'kernel': f'{dom}: PyTorch-ROCm CRNN forward ({"bf16" if dnn_dtype is not None else "float32"} rocBLAS GEMMs + MIOpen convolutions, not a kernel of this library)',
                        'achieved': round(achieved / 1e12, 2), 'peak': peak / 1e12, 'unit': 'TFLOP/s',
                        'frac': round(achieved / peak, 4), 'traffic': None, 'avg_launch_ms': round(launch_ms, 4),
                        'flops_per_launch': stages[dom]['flops'] / lps, 'pipeline': pipeline}
        else:
            cand = [n_ for n_ in stages if 'alg_bytes' in stages[n_]]
            dom = max(cand, key=lambda n_: stages[n_]['ms'])
            lps = stages[dom]['launches_per_step']
            launch_ms = stages[dom]['ms'] / lps
            launch_bytes = stages[dom]['alg_bytes'] / lps
            achieved = launch_bytes / (launch_ms * 1e-3)
            traffic, traffic_note = None, None
            tfile = os.path.join(REPO, 'profiles', f'pmc_traffic_{name}.json')
            if os.path.exists(tfile):
                try:
                    tj = json.load(open(tfile))
                    traffic = tj.get(dom, {}).get('hbm_bytes_per_launch')
                    if tj.get('_csrc_digest') != csrc_digest():
                        traffic_note = (f'{os.path.basename(tfile)} was measured on other kernel sources (digest '
                                        f'{tj.get("_csrc_digest")} vs {csrc_digest()}): stale, shown for orientation only')
                except Exception:
                    traffic = None
            roofline = {'bound': 'hbm', 'kernel': dom, 'achieved': round(achieved / 1e9, 1), 'peak': HBM_PEAK / 1e9,
                        'unit': 'GB/s', 'frac': round(achieved / HBM_PEAK, 4), 'traffic': traffic,
                        'alg_bytes_per_launch': launch_bytes, 'avg_launch_ms': round(launch_ms, 4), 'pipeline': pipeline,
                        'measured': 'HIP events around every stage, kernels one at a time (option overlap_solves = 0 for this pass; '
                                    f'the timed region ran with overlap_solves = {overlap_was}); pipeline = whole path over the timed region'}
            if online_every > 0:
                roofline['note'] = ('the online kernels re-solve a P x P GEVD per (bin, frame): float64-issue-bound, not HBM-bound; the '
                                    'fraction says how far they are from the streaming bound of their inputs')
                # the bound that applies: VALU issue.  SQ_INSTS_VALU of the dominant online kernel (profiles/pmc_alu_<name>.json, taken with
                # tools/gpu/pmc_alu.sh on these sources) against the issue slots of its launch: 1024 SIMDs x 2.4 GHz, one wave64
                # instruction per 4 cycles (float32 / packed) or 8 (float64 multiply-adds: half rate) -- the truth lies between the two
                afile = os.path.join(REPO, 'profiles', f'pmc_alu_{name}.json')
                if os.path.exists(afile):
                    try:
                        aj = json.load(open(afile))
                        kk = [k_ for k_ in aj if 'k_online_mwf' in k_ and f'<{M + K - 1},' in k_]
                        if kk:
                            insts = aj[kk[0]]['SQ_INSTS_VALU']['per_dispatch']
                            slots = 1024 * 2.4e9 * (launch_ms * 1e-3)
                            roofline['valu_issue'] = {'kernel': kk[0][:60], 'valu_insts_per_launch': insts,
                                                      'frac_of_issue_slots_at_4_cycles': round(insts * 4 / slots, 3),
                                                      'frac_of_issue_slots_at_8_cycles': round(insts * 8 / slots, 3),
                                                      'stale': aj.get('_csrc_digest') != csrc_digest(),
                                                      'what': 'SQ_INSTS_VALU x cycles per wave64 instruction / (1024 SIMDs x 2.4 GHz x launch time)'}
                    except Exception:
                        pass
            if traffic_note:
                roofline['traffic_note'] = traffic_note
            elif traffic is not None and traffic < 0.9 * launch_bytes:
                sanity.append(f'{dom}: counter traffic {traffic:.3e} B per launch is below 0.9 x the algorithmic bytes {launch_bytes:.3e}: byte model or counters wrong')
            if dom in ('stft_cov1', 'stft'):
                roofline['byte_model_note'] = ('the byte model of this kernel includes the store of the spectra X (8 M F per node-frame), which SURVEY 8(d) '
                                               'treats as avoidable (STFT recomputed, not stored); the 8(d)-faithful figure is `pipeline`')
        if sanity:
            roofline = dict(roofline or {}, sanity_errors=sanity)

    exchange = None
    if node_sharded:
        exchange = exchange_object(R, K, Kl, T, F, iters, gather_ms, world, args.overlap_exchange,
                                   ('separate pass after the timed region, overlap off: whole batch per gather' if args.full
                                    else 'not timed: overlapped gathers are timed in a separate pass (--full)') if args.overlap_exchange
                                   else 'inside the timed region: one whole-batch gather per step-2 iteration')

    mask_error = None
    if dnn_dtype is not None:
        # what the low-precision operands cost: the same networks evaluated in float32 on the same batch
        _, mz32, mw32 = tango_enhance_dnn(eng, y, model_z, model_w, want_masks=True)
        mask_error = {'vs': 'the float32 evaluation of the same networks on the same batch',
                      'mask_z_max_abs': float((dnn['mz'] - mz32).abs().max()), 'mask_z_mean_abs': float((dnn['mz'] - mz32).abs().mean()),
                      'mask_w_max_abs': float((dnn['mw'] - mw32).abs().max()), 'mask_w_mean_abs': float((dnn['mw'] - mw32).abs().mean())}
        del mz32, mw32
    stream = None
    if online_every > 0 and rank == 0 and not node_sharded and not args.no_stage_timing:      # (counter passes run the whole-clip launch alone)
        try:
            stream = stream_bench(eng, lib, torch, y, mask, online_every, H, F)
        except Exception as e:                              # reported, never fatal: the whole-clip numbers above stand on their own
            stream = {'error': repr(e)}
    mask_desc = 'oracle irm1 mask' if mask_kind == 'oracle' else ('CRNN masks in the loop (random weights, PyTorch-ROCm' + (', convolutions / GEMMs on bf16 operands)' if dnn_dtype is not None else ')'))
    par = (f'nodes of every room split over {world} GPU(s) ({Kl} per rank), one RCCL all-gather of z per step-2 iteration'
           if node_sharded else f'rooms sharded over {world} GPU(s), no data-path collective')
    res = {
        'value': value, 'unit': 'node-frames/s', 'ms_per_step': ms_per_step, 'x_realtime': x_rt, 'steps': steps, 'warmup': warmup,
        'seconds_local': dt_local, 'units_local': units_per_step * steps,
        'config': {'workload': f'{name}: {R} rooms{"" if node_sharded else "/GPU"} x {K} nodes x {M} mics, 16 kHz, L={Ls}, '
                               f'{N}-pt STFT hop {H}, {mask_desc}, two-step Tango (mask_for_z=local), outputs=enhanced'
                               + (f', ONLINE mode lambda=0.95 update_every={online_every}' if online_every else '')
                               + (f', {iters} step-2 iterations (DANSE-style)' if iters > 1 else ''),
                   'launch': 'one hipGraph replay per step' if (args.graph and headline) else 'eager kernel launches',
                   'rooms_per_gpu': R, 'nodes': K, 'mics': M, 'length': Ls, 'n_fft': N, 'frames': T,
                   'iters': iters, 'parallelism': par},
        'roofline': roofline, 'stages': stages,
    }
    if stream:
        res['stream'] = stream
    if graph_res:
        res['graph'] = graph_res
    if exchange:
        res['exchange'] = exchange
    if mask_error:
        res['mask_error'] = mask_error
    del y, s_ref, n_ref, mask, out, ws, eng
    torch.cuda.empty_cache()
    return res, ticket


def stream_bench(eng, lib, torch, y, mask, update_every, H, F, chunk_hops=(1, 4, 16), audio_hops=64):
    """The STREAMING entry point (disco_tango_online_stream: state in, state out; SURVEY 8f-2 "streaming latency instead of batch") on the
    batch the whole-clip call was just timed on: after a 16-hop start, `audio_hops` hops of every room are pushed in chunks of 1, 4 and 16
    hops -> ms per chunk and x real-time (audio time of a chunk / wall time of a chunk: > 1 means the stream keeps up with 1000 live rooms).
    A chunk's inputs (its samples, its mask rows) are sliced out BEFORE the clock starts -- a live caller hands over exactly such blocks.
    The bit-for-bit equality of the chunked and the whole-clip outputs is tests/ business (check_online_stream), not repeated here."""
    R, K, M, L = y.shape
    state = torch.empty(int(lib.disco_online_state_bytes(eng.ctx)), dtype=torch.uint8, device=y.device)
    start = 16
    out = {'chunks': {}, 'rooms': R, 'update_every': update_every, 'hop_ms': 1e3 * H / 16000.0,
           'what': f'disco_tango_online_stream, {R} concurrent rooms, {audio_hops} hops of audio per chunk size after a {start}-hop start; '
                   'latency of an output sample = one hop (the centred frame) + the chunk + ms_per_chunk'}
    for hops in chunk_hops:
        ws = torch.empty(int(lib.disco_online_stream_workspace_bytes(eng.ctx, max(hops, start))), dtype=torch.uint8, device=y.device)
        o = torch.empty((R, K, max(hops, start) * H), dtype=torch.float32, device=y.device)

        def push(h0, n):
            yc = y[:, :, :, h0 * H:(h0 + n) * H].contiguous()
            mc = mask[:, :, h0:h0 + n].contiguous()
            return yc, mc
        y0, m0 = push(0, start)
        eng._chk(lib.disco_tango_online_stream(eng.ctx, y0.data_ptr(), start, m0.data_ptr(), m0.data_ptr(), 0.95, update_every, 1e-3, 0, 0,
                                               state.data_ptr(), o.data_ptr(), ws.data_ptr(), ws.numel(), None))
        n_chunks = max(2, audio_hops // hops)
        blocks = [push(start + i * hops, hops) for i in range(n_chunks)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (yc, mc) in enumerate(blocks):
            eng._chk(lib.disco_tango_online_stream(eng.ctx, yc.data_ptr(), hops, mc.data_ptr(), mc.data_ptr(), 0.95, update_every, 1e-3,
                                                   start + i * hops, 0, state.data_ptr(), o.data_ptr(), ws.data_ptr(), ws.numel(), None))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n_chunks
        out['chunks'][str(hops)] = {'ms_per_chunk': round(1e3 * dt, 3), 'chunk_audio_ms': round(1e3 * hops * H / 16000.0, 2),
                                    'x_realtime': round((hops * H / 16000.0) / dt, 2), 'chunks_timed': n_chunks,
                                    'node_frames_per_s': round(R * K * hops / dt, 1),
                                    'finite': bool(torch.isfinite(o[:, :, :hops * H]).all())}
        del blocks, ws, o
    return out


def finish_parity(ticket, env, timeout=900.0):
    """Wait for this rank's oracle jobs of one workload, then merge over the ranks -> parity_sample object (same on every rank)."""
    rank, world = env['rank'], env['world']
    per_room, worst, err, flagged = {}, 0.0, None, {}
    for fut in ticket['jobs']:
        try:
            res_ = fut.result(timeout=timeout)
            room, e = res_[0], res_[1]
            if len(res_) > 2 and res_[2].get('flagged_bins'):
                flagged[int(room)] = res_[2]
        except Exception as ex:                            # a checker that cannot run is a failed check, not a silent pass
            room, e, err = -1, float('inf'), repr(ex)
        per_room[int(room)] = e
        worst = max(worst, e)
    if not ticket['finite']:
        worst = float('inf')
    rows = gather_rank_rows(rank, world, env['local_rank'], ticket['first_room'], ticket['rooms_global'], worst, env['dist'], env['cdev'])
    ps = merge_parity({'rooms': ticket['rooms_global'], 'per_room': per_room, 'worst_rel': worst}, rows, ticket['tol'])
    if err:
        ps['error'] = err
    if flagged:
        ps['flagged'] = {'rooms': flagged, 'criterion': f'a bin is flagged when the float64 oracle\'s own output in it moves by more than tol / {1 / FLAG_SENS:g} under a float32-class '
                         f'perturbation of its inputs (masks by one float32 rounding, samples by {F32_SAMPLE_NOISE:g}) or a statistic has less than {FLAG_WEIGHT:g} frames of '
                         'weight; unflagged bins at tol per node; flagged bins per node E_hip <= max(tol ||yf||, 2 E_ref32), E_ref32 = the distance of the reference\'s own '
                         'arithmetic (complex64 statistics, scipy.linalg.eig + clamps) from the same oracle -- bench.py score_given_masks'}
    return ps


def merge_extras(res, env):
    """value of an extra workload over the whole job: units of all ranks / the slowest rank's time (every rank on its own clock)."""
    import torch
    world = env['world']
    if world == 1:
        return res
    t = torch.tensor([res['seconds_local'], res['units_local']], dtype=torch.float64, device=env['cdev'])
    outs = [torch.empty_like(t) for _ in range(world)]
    env['dist'].all_gather(outs, t)
    secs = [float(o[0]) for o in outs]
    units = sum(float(o[1]) for o in outs)
    res['value'] = units / max(secs)
    res['ms_per_step'] = 1e3 * max(secs) / res['steps']
    res['x_realtime'] = (res['config']['length'] / 16000.0) / (max(secs) / res['steps'])
    res['seconds_per_rank'] = secs
    return res


def summary_rows(head_name, head, head_parity, extras):
    """{workload: [ms_per_step, x_realtime, pipeline_frac, dominant_kernel, dominant_frac, traffic_ratio, parity_worst]} -- traffic_ratio =
    counter traffic / algorithmic bytes of the dominant kernel (None when the counters were taken on other kernel sources)."""
    def row(r, ps):
        rf = r.get('roofline') or {}
        tr = None
        if rf.get('traffic') and rf.get('alg_bytes_per_launch') and 'traffic_note' not in rf:
            tr = round(rf['traffic'] / rf['alg_bytes_per_launch'], 3)
        kern = str(rf.get('kernel', ''))[:24]
        out = [round(r['ms_per_step'], 3), round(r['x_realtime'], 1), (rf.get('pipeline') or {}).get('frac'), kern, rf.get('frac'), tr,
               None if ps is None else float('%.3g' % ps.get('worst_rel_all_ranks', float('nan')))]
        if 'stream' in r:       # the streaming entry point: x real-time at chunks of 1 / 4 / 16 hops
            out.append({'stream_x_realtime_by_hops': {k: v.get('x_realtime') for k, v in r['stream'].get('chunks', {}).items()}})
        if 'graph' in r:        # the same step as one hipGraph replay: [ms_per_step, pipeline_frac]
            out.append({'hipgraph': [r['graph'].get('ms_per_step'), r['graph'].get('pipeline_frac')]})
        if ps and ps.get('flagged'):        # rooms with bins whose PREDICTED masks leave a statistic without frames: asserted against the reference's own noise
            fl = ps['flagged']['rooms']
            out.append({'rooms_with_flagged_bins': [len(fl), len(ps.get('per_room', {}))],
                        'worst_E_hip/max(tol|yf|,2E_ref32)': float('%.3g' % max(v.get('flagged_ratio', 0.0) for v in fl.values())),
                        'worst_unflagged_rel': float('%.3g' % max(v.get('unflagged_rel', 0.0) for v in fl.values()))})
        return out
    rows = {'_cols': 'ms_per_step, x_realtime, pipeline_frac, dominant_kernel, dominant_frac_of_peak, traffic/alg_bytes, parity_worst_rel[, {stream x_realtime by chunk hops}][, {hipgraph: [ms_per_step, pipeline_frac]}][, {rooms_with_flagged_bins: [n, of sampled], worst E_hip / max(tol |yf|, 2 E_ref32) over the flagged bins of a node (asserted <= 1), worst error over the unflagged bins (asserted < tol)}]',
            head_name: row(head, head_parity)}
    for nm, r in extras.items():
        rows[nm] = row(r, r.get('parity_sample')) if 'error' not in r else 'error'
    return rows


LINE_LIMIT = 6000     # bytes of the ONE stdout line (tests/test_bench_line_cpu.py); the driver stopped parsing somewhere between 17 and 20 kB


def _short(x, digits=4):
    """Numbers of the compact line: 4 significant digits for fractions / errors, plain ints kept."""
    if isinstance(x, float):
        return float(f'%.{digits}g' % x) if x == x and abs(x) != float('inf') else None
    return x


def compact_line(full, detail_path=None):
    """The ONE stdout line from the full result: the contract's keys first, `roofline` and `cpu_baseline` with their numbers and NO
    prose, the parity verdict, the path of the side file, and `summary` (every workload's numbers) last.  Stages, per-room errors,
    per-rank rows, notes and the attached configurations live in the side file (bench_detail.json)."""
    line = {k: full[k] for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                                 'vs_baseline', 'dtype', 'data', 'x_realtime')}
    c = full['config']
    line['config'] = {k: c[k] for k in ('workload', 'launch', 'rooms_per_gpu', 'nodes', 'mics', 'length', 'n_fft', 'frames', 'iters',
                                        'parallelism') if k in c}
    rf = full.get('roofline')
    if rf:
        out = {k: rf.get(k) for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'traffic')}
        out['kernel'] = str(out['kernel'])[:48]
        for k in ('alg_bytes_per_launch', 'flops_per_launch', 'avg_launch_ms'):
            if k in rf:
                out[k] = rf[k]
        if rf.get('pipeline'):
            out['pipeline'] = rf['pipeline']
        if rf.get('sanity_errors'):
            out['sanity_errors'] = len(rf['sanity_errors'])
        if 'traffic_note' in rf:
            out['traffic_stale'] = True
        line['roofline'] = out
    else:
        line['roofline'] = None
    cb = full.get('cpu_baseline')
    if cb:
        out = {'value': _short(cb['value']), 'unit': cb['unit'], 'cores': cb['cores'], 'kind': cb['kind'], 'sample': cb['sample'][:200],
               'x_realtime': _short(cb.get('x_realtime'))}
        for k in ('vectorised_numpy', 'vectorised_numpy_all_cores'):
            v = cb.get(k)
            if v and 'value' in v:
                out[k] = {'value': _short(v['value']), 'cores': v.get('cores', 1)}
        line['cpu_baseline'] = out
    else:
        line['cpu_baseline'] = None
    ps = full.get('parity_sample')
    if ps:
        line['parity_sample'] = {'rooms_checked': sum(len(r['rooms_checked']) for r in ps['ranks']), 'ranks': len(ps['ranks']),
                                 'worst_rel_all_ranks': _short(ps['worst_rel_all_ranks']), 'tol': ps['tol'], 'ok': ps['ok'],
                                 'oracle': 'float64 CPU oracle (oracle/tango_oracle.py), last timed step'}
        if 'error' in ps:
            line['parity_sample']['error'] = str(ps['error'])[:120]
    ex = full.get('exchange')
    if ex:
        line['exchange'] = {k: _short(ex.get(k)) for k in ('collective', 'gathers_per_step', 'bytes_received_per_rank_per_gather',
                                                           'bytes_per_peer_link_per_gather', 'ms_per_gather', 'link_GBps', 'timed')}
    if 'graph' in full:
        line['graph'] = {k: full['graph'].get(k) for k in ('ms_per_step', 'pipeline_frac', 'error') if k in full['graph']}
    if detail_path:
        line['detail'] = detail_path
    line['summary'] = full['summary']        # LAST key
    n = len(json.dumps(line))
    if n > LINE_LIMIT:                       # never again an unparsed line: shed the optional parts, then the summary's column legend
        for k in ('graph', 'exchange'):
            line.pop(k, None)
        line['summary'] = {k: v for k, v in line['summary'].items() if k != '_cols'}
    assert len(json.dumps(line)) <= LINE_LIMIT, len(json.dumps(line))
    return line


def write_detail(full, path=None):
    """The full result (stages, per-room parity, per-rank rows, notes, every attached configuration) as ONE json file: `path`, else
    bench_detail.json at the repo root and -- when the directory exists (a gpurun call) -- gpurun_out/bench_detail.json.  A side file
    that cannot be written is reported on stderr and never fails the bench.  -> the paths written (repo-relative)."""
    targets = [path] if path else [os.path.join(REPO, 'bench_detail.json')]
    if not path and os.path.isdir(os.path.join(REPO, 'gpurun_out')):
        targets.append(os.path.join(REPO, 'gpurun_out', 'bench_detail.json'))
    done = []
    for t in targets:
        try:
            with open(t, 'w') as f:
                json.dump(full, f, indent=1)
                f.write('\n')
            done.append(os.path.relpath(t, REPO))
        except OSError as e:
            print(f'bench detail file {t}: {e!r}', file=sys.stderr)
    return done


def dump_outputs(out_dir, arrays, budget=DUMP_BYTES, seed=0):
    """--dump-outputs: `arrays` (name -> tensor, the room as leading axis) as out_dir/<name>.npy in float32, at most `budget` bytes in all.
    Every array keeps the same rooms: all of them when they fit, else a fixed seeded sample (ascending).  When one room alone is over the
    budget, each array is cut further to a fixed seeded sample of its elements (ascending flat indices), in proportion to its size.
    -> the rooms written."""
    import numpy as np
    import torch
    R = next(iter(arrays.values())).shape[0]
    per_room = sum(4 * a[0].numel() for a in arrays.values())
    n = min(R, budget // per_room)
    rng = np.random.default_rng(seed)
    rooms = np.arange(R) if n == R else np.sort(rng.choice(R, max(n, 1), replace=False))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        x = a.index_select(0, torch.as_tensor(rooms, device=a.device))
        if n == 0:
            keep = budget * a[0].numel() // per_room
            x = x.reshape(-1)[torch.as_tensor(np.sort(rng.choice(x.numel(), keep, replace=False)), device=a.device)]
        np.save(os.path.join(out_dir, name + '.npy'), x.float().cpu().numpy())
    return rooms.tolist()


def exchange_object(R, K, Kl, T, F, iters, gather_ms, world, overlap, timed):
    """The line's `exchange` object (--shard nodes): one all-gather of z per step-2 iteration; every rank receives the other ranks' z
    (R (K - Kl) T F complex64) and sends its own R Kl T F block to each peer over that peer's link (xGMI is point-to-point)."""
    per_gather = R * (K - Kl) * T * F * 8
    ms = (sum(gather_ms) / len(gather_ms)) if gather_ms else None
    return {'collective': 'all_gather_into_tensor (RCCL)', 'gathers_per_step': 2 * iters if overlap else iters, 'timed': timed, 'overlap': bool(overlap),
            'bytes_received_per_rank_per_gather': per_gather, 'bytes_per_peer_link_per_gather': R * Kl * T * F * 8, 'ms_per_gather': ms,
            'link_GBps': (R * Kl * T * F * 8 / (ms * 1e-3) / 1e9) if (ms and world > 1) else None,
            'note': 'xGMI is point-to-point: each of the W-1 peers sends its R*Kl*T*F*8-byte block over its own link'}


def dry_collective(args, rank, world, emit):
    """--dry-collective: the exchange of the node-sharded step over gloo on CPU tensors (no GPU, no kernels): rank r fills its (R, Kl, T, F)
    block with a value that encodes (rank, iteration), all ranks all-gather `iters` times per step into the rank-major [W][R][Kl][T][F]
    buffer the kernels consume in place (Engine.set_z_blocks), every rank checks every block, rank 0 prints the exchange object."""
    import torch
    from disco_amd import dist as dd
    from disco_amd import node_sharded as ns
    if args.shard != 'nodes':
        raise SystemExit('--dry-collective exercises the z exchange: use it with --shard nodes')
    dist = dd.init('gloo', rank, world)
    R, K, N, iters = args.rooms, args.nodes, args.n_fft, args.iters
    T, F = 1 + args.length // (N // 2), N // 2 + 1
    k0, Kl = ns.node_range(rank, world, K)
    z = torch.empty((R, Kl, T, F, 2), dtype=torch.float32)
    parts = torch.empty((world * R, Kl, T, F, 2), dtype=torch.float32)
    gather_ms, bad = [], 0
    for step in range(args.warmup + args.steps):
        for it in range(iters):
            z.fill_(float(1000 * rank + 10 * step + it))
            dist.barrier()
            t0 = time.perf_counter()
            dist.all_gather_into_tensor(parts, z)
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                gather_ms.append(1e3 * dt)
            got = parts.view(world, R, Kl, T, F, 2)
            bad += sum(int(not bool((got[w_] == float(1000 * w_ + 10 * step + it)).all())) for w_ in range(world))
    flag = torch.tensor([float(bad)], dtype=torch.float64)
    dist.all_reduce(flag)
    ex = exchange_object(R, K, Kl, T, F, iters, gather_ms, world, False,
                         'DRY RUN: gloo on CPU tensors of the real per-rank size, no kernels: bookkeeping of the exchange, not a measurement')
    ex['collective'] = 'all_gather_into_tensor (gloo, dry run)'
    if rank == 0:
        emit({'selftest': 'dry-collective', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'scaling': 'strong',
              'config': {'rooms': R, 'nodes': K, 'nodes_per_rank': Kl, 'frames': T, 'bins': F, 'iters': iters}, 'blocks_wrong': int(flag.item()),
              'gathers_timed': len(gather_ms), 'exchange': ex})
    dist.barrier()
    dist.destroy_process_group()
    return 0 if flag.item() == 0 else 5


def main(argv=None):
    args = parse_args(argv)
    from disco_amd import dist as dd
    rank, world, local_rank = dd.env_rank_world()
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        # started plainly: become the launcher of N ranks of this very command line (one process per GPU)
        # (with --single-device the launcher leaves the GPU alone: counting devices would open it in one more process than the ranks)
        if not (args.selftest_launch or args.dry_collective or args.single_device):
            import torch
            have = torch.cuda.device_count()
            if have < args.gpus:
                raise SystemExit(f'--gpus {args.gpus} but only {have} GPU(s) are visible')
        raise SystemExit(dd.launch_ranks(os.path.abspath(__file__), sys.argv[1:] if argv is None else list(argv), args.gpus))
    if args.gpus != world:
        raise SystemExit(f'--gpus {args.gpus} but WORLD_SIZE {world}: start with --gpus {world}, or plainly (no torchrun) to self-launch')

    # The ONE JSON line is the only thing this process may put on stdout: libraries print banners there (RCCL its version block, from C
    # stdio, flushed at exit -- i.e. AFTER the line).  The original stdout is kept for the line; descriptor 1 becomes stderr for everybody else.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    def emit(obj):
        os.write(json_fd, (json.dumps(obj) + '\n').encode())

    if args.dry_collective:
        return dry_collective(args, rank, world, emit)
    if args.selftest_launch:
        dist = dd.init('gloo', rank, world)
        value, dt = dd.whole_job_throughput(1000.0 * (rank + 1), 0.5 + 0.1 * rank, world)
        # the all-rank parity bookkeeping on fake numbers: rank r "checked" its rooms with worst error 1e-6 * (r + 1)
        rooms = [10 * rank + x for x in rank_sample_rooms(rank, 10, 3)]
        rows = gather_rank_rows(rank, world, local_rank, 10 * rank, rooms, 1e-6 * (rank + 1), dist, 'cpu', gloo=True)
        ps = merge_parity({'rooms': rooms, 'per_room': {r: 1e-6 * (rank + 1) for r in rooms}, 'worst_rel': 1e-6 * (rank + 1)}, rows, 1e-4)
        if rank == 0:
            emit({'selftest': 'launch', 'n_gpus': world, 'value': value, 'seconds': dt, 'parity_sample': ps})
        dist.barrier()
        dist.destroy_process_group()
        return 0

    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor

    import torch
    from disco_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X: there is no CPU path')
    dev_index = 0 if args.single_device else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device('cuda', dev_index)
    cdev = dev if args.dist_backend == 'nccl' else torch.device('cpu')        # where the control collectives' tensors live
    node_sharded = args.shard == 'nodes'
    if world == 1 and node_sharded:
        os.environ.setdefault('MASTER_PORT', str(dd.free_port()))
    dist = dd.init(args.dist_backend, rank, world, device=dev) if (world > 1 or node_sharded) else None    # RCCL (one-rank group for --shard nodes)
    lib = _lib.load()
    # oracle workers: fresh interpreters (spawn: a forked HIP context is not usable), single-threaded numpy each
    for v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
        os.environ.setdefault(v, '1')
    pool = None if args.no_parity else ProcessPoolExecutor(max_workers=max(2, min(args.parity_workers, (os.cpu_count() or 8) // max(world, 1))),
                                                           mp_context=mp.get_context('spawn'))
    import tempfile
    tmpdir = tempfile.mkdtemp(prefix='disco_bench_')
    env = dict(rank=rank, world=world, local_rank=dev_index, dev=dev, cdev=cdev, dist=dist, lib=lib, pool=pool, tmpdir=tmpdir)

    head_w = {k: getattr(args, k) for k in ('rooms', 'nodes', 'mics', 'n_fft', 'iters', 'mask', 'online_every')}
    cfg_shape = CONFIGS[args.config]
    is_cfg = all(head_w[k] == cfg_shape[k] for k in ('nodes', 'mics', 'n_fft', 'iters', 'mask', 'online_every'))
    head_name = args.config if is_cfg else 'custom'
    n_par = args.parity_rooms        # (an 8 x 8 room costs the oracle ~11 s on one core: the default of 6 stays; sweeps raise --parity-workers)
    head, head_ticket = run_workload(head_name, head_w, args.steps, args.warmup, env, True, n_par, args)

    extras, tickets = {}, {}
    for nm in args.extra_names:
        w, st, wu, npar = EXTRAS[nm]
        try:
            extras[nm], tickets[nm] = run_workload(nm, w, min(st, max(args.steps, 1)), min(wu, args.warmup), env, False, npar, args)
        except Exception as e:                              # an extra must never take the headline down
            import traceback
            extras[nm] = {'error': repr(e), 'trace': traceback.format_exc()[-1500:]}
            torch.cuda.empty_cache()

    # ---- collect: parity of every workload (all ranks), whole-job value of the extras
    parity = None if args.no_parity else finish_parity(head_ticket, env)
    failures, soft_failures = [], []       # headline: fails the command; extras: reported in the line and on stderr only
    if parity is not None and not parity['ok']:
        failures.append((head_name, parity['worst_rel_all_ranks']))
    for nm in args.extra_names:
        # every rank takes part in the same gathers in the same order, whether its own run of the extra succeeded or not
        ok_local = 'error' not in extras[nm]
        if world > 1:
            flag = torch.tensor([1.0 if ok_local else 0.0], dtype=torch.float64, device=cdev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            all_ok = bool(flag.item() > 0.5)
        else:
            all_ok = ok_local
        if not all_ok:
            if ok_local:
                extras[nm] = {'error': 'another rank failed this workload'}
            continue
        extras[nm] = merge_extras(extras[nm], env)
        if not args.no_parity:
            extras[nm]['parity_sample'] = finish_parity(tickets[nm], env)
            if not extras[nm]['parity_sample']['ok']:
                soft_failures.append((nm, extras[nm]['parity_sample']['worst_rel_all_ranks']))
        for k in ('seconds_local', 'units_local'):
            extras[nm].pop(k, None)
    if pool is not None:
        pool.shutdown(wait=True)
    import shutil
    shutil.rmtree(tmpdir, ignore_errors=True)

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(head_w['nodes'], head_w['mics'], args.length, head_w['n_fft'])

    if rank == 0:
        full = {
            'metric': 'STFT node-frames/s, whole MWF path (STFT->mask->cov->GEVD-MWF->z exchange->MWF->iSTFT)',
            'value': head['value'], 'unit': 'node-frames/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': head['ms_per_step'], 'higher_is_better': True, 'scaling': 'strong' if node_sharded else 'weak',
            'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'x_realtime': head['x_realtime'],
            'config': head['config'],
            'roofline': head['roofline'], 'cpu_baseline': cpu, 'parity_sample': parity, 'stages': head['stages'],
        }
        for extra_key in ('exchange', 'stream', 'graph'):
            if extra_key in head:
                full[extra_key] = head[extra_key]
        if args.extra_names:
            full['configs'] = extras
        full['summary'] = summary_rows(head_name, head, parity, extras)
        # everything goes to the side file; stdout carries the compact line (a 20 kB line was not parsed)
        detail_paths = write_detail(full, args.detail)
        line = compact_line(full, detail_paths[0] if detail_paths else None)
        emit(line)
    if dist is not None:
        dist.barrier()                    # leave together
        dist.destroy_process_group()
    for nm, worst in failures + soft_failures:
        print(f'PARITY FAILURE ({nm}): worst relative error over all ranks {worst:.3e} >= {PARITY_TOL:.1e}', file=sys.stderr)
    sanity = [(nm, e) for nm, r_ in [(head_name, head)] + [(n_, x_) for n_, x_ in extras.items() if 'error' not in x_]
              for e in ((r_.get('roofline') or {}).get('sanity_errors') or [])] if rank == 0 else []
    for nm, e in sanity:
        print(f'SANITY FAILURE ({nm}): {e}', file=sys.stderr)
    # exit code: 3 = the headline failed its parity bar (or a sanity check of its byte models), 4 = an attached workload did; the line is
    # printed either way
    if failures or any(nm == head_name for nm, _ in sanity):
        return 3
    return 4 if (soft_failures or sanity) else 0


if __name__ == '__main__':
    sys.exit(main())
