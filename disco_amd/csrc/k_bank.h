// Filling the training bank from rooms (disco_amd/dnn/data.py SpectraBank.from_rooms): the magnitudes of the mixture spectra at the reference
// microphone and of the compressed signals, and the label masks, of R rooms written into R consecutive segments of bank [S][N][Tb][F] in one launch.
//
// A streaming kernel: per (room, frame, bin) it reads (8 (1 + n_zsig) + 4) K bytes and writes 4 S, each source element once and each bank element once.
// The map follows from the layouts.  The frames [skip, skip + n) of one (room, node) plane of z or of the mask are n F CONSECUTIVE elements, and so are the
// frames [0, n) of the bank plane (row, segment) they go to: a bank plane is a linear copy of a run of its source plane followed by zeros, and no element
// needs its (frame, bin) at all -- no division per element (a flat index over the whole bank costs three 64-bit divisions per element, which at the
// bank's 0.3 G elements per 125 ten-second rooms is more arithmetic than the copy is memory traffic).  One workgroup column (blockIdx.x) owns one bank
// plane; its row, room and source are scalar values.  Lanes take consecutive elements: a wave reads 512 consecutive bytes (complex) or 256 (mask) and
// writes 256 consecutive bytes per instruction.  Wider accesses were not taken: F = 257 is odd, so a plane starts on a 4-byte boundary (8 for the complex
// sources) and 16-byte accesses would need a peeled head and tail per plane on both sides with different phases.  BANK_UNROLL independent loads per lane
// are in flight before the first store.  The mixture's spectra X [R][K][T][F][M] are read at one microphone: 8 of every 8 M bytes of the lines fetched.
#pragma once
#include "common.h"

namespace disco {

constexpr int BANK_THREADS = 256;
constexpr int BANK_UNROLL = 4;
constexpr int BANK_CHUNK = BANK_THREADS * BANK_UNROLL;      // elements of a plane one workgroup handles per pass

// Row order (SpectraBank): row k the mixture of node k, row K (1 + i) + k z signal i of node k, row K (1 + n_zsig) + k the mask of node k.
// za, zb: the z signals present, in order (zb only for n_zsig == 2).  frames [R] or nullptr (= T); a value above T counts as T.
// Bank frame tb of segment seg0 + r = source frame tb + skip while tb + skip < min(frames[r], T), else +0.f; every tb < Tb is written.
// grid (S R, chunks), block BANK_THREADS.
static __global__ void __launch_bounds__(BANK_THREADS)
k_bank_fill(const c32* __restrict__ X, const c32* __restrict__ za, const c32* __restrict__ zb, const float* __restrict__ mask,
            const int* __restrict__ frames, float* __restrict__ bank, int R, int K, int M, int T, int F, int mic, int n_zsig, int skip, long long N,
            int Tb, long long seg0) {
    const long long plane = blockIdx.x;                     // row * R + r: the planes of a row's R segments are consecutive in the bank
    const int row = (int)(plane / R), r = (int)(plane - (long long)row * R);
    const int kind = row / K, k = row - kind * K;           // 0: mixture, 1 ... n_zsig: z signal kind - 1, n_zsig + 1: mask
    int nf = frames ? frames[r] : T;
    nf = (nf < T ? nf : T) - skip;                          // frames this room gives the bank ...
    nf = nf < 0 ? 0 : (nf < Tb ? nf : Tb);                  // ... in [0, Tb]
    const long long len = (long long)Tb * F, valid = (long long)nf * F;
    const long long src = (((long long)r * K + k) * T + skip) * F;      // frame `skip` of the source plane (read only below `valid`)
    float* __restrict__ dst = bank + (((long long)row * N + seg0 + r) * Tb) * F;
    const c32* __restrict__ z = kind == 1 ? za : zb;
    for (long long e0 = (long long)blockIdx.y * BANK_CHUNK + threadIdx.x; e0 < len; e0 += (long long)gridDim.y * BANK_CHUNK) {
        float v[BANK_UNROLL];
#pragma unroll
        for (int j = 0; j < BANK_UNROLL; ++j) {
            const long long e = e0 + j * BANK_THREADS;
            v[j] = 0.f;
            if (e < valid) {
                if (kind == 0)
                    v[j] = cabs_fma(X[(src + e) * M + mic]);
                else if (kind <= n_zsig)
                    v[j] = cabs_fma(z[src + e]);
                else
                    v[j] = mask[src + e];                   // the bits as they are: no abs
            }
        }
#pragma unroll
        for (int j = 0; j < BANK_UNROLL; ++j) {
            const long long e = e0 + j * BANK_THREADS;
            if (e < len) dst[e] = v[j];
        }
    }
}

}  // namespace disco
