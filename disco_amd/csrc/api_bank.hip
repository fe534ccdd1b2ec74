// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): the training bank filled from rooms (k_bank.h)
#include "host.h"
#include "k_bank.h"

using namespace disco;
using namespace disco_host;

extern "C" int disco_bank_fill(disco_ctx* ctx, const disco_c32* X, const disco_c32* z0, const disco_c32* z1, const float* mask, const int32_t* frames,
                               int64_t R, int K, int M, int T, int F, int mic, int n_zsig, int skip, float* bank, int64_t N, int Tb, int64_t seg0,
                               disco_stream s) {
    if (!X || !mask || !bank || R < 1 || K < 1 || M < 1 || T < 1 || F < 1 || mic < 0 || mic >= M || skip < 0 || Tb < 1 || N < 1 || seg0 < 0 ||
        seg0 > N - R || n_zsig != (z0 != nullptr) + (z1 != nullptr))
        return fail(ctx, DISCO_E_ARG, "disco_bank_fill: bad argument");
    const long long planes = (long long)R * K * (2 + n_zsig);
    if (planes > 0x7fffffffLL || R > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_bank_fill: too many planes for one launch");
    DevGuard dev_guard_(current_device(ctx));
    const long long chunks = ((long long)Tb * F + BANK_CHUNK - 1) / BANK_CHUNK;
    const c32* za = (const c32*)(z0 ? z0 : z1);             // the z signals present, in order
    const c32* zb = (const c32*)(z0 ? z1 : nullptr);
    hipLaunchKernelGGL(k_bank_fill, dim3((unsigned)planes, (unsigned)std::min<long long>(chunks, 256)), dim3(BANK_THREADS), 0, (hipStream_t)s,
                       (const c32*)X, za, zb, mask, (const int*)frames, bank, (int)R, K, M, T, F, mic, n_zsig, skip, (long long)N, Tb, (long long)seg0);
    return launched();
}
