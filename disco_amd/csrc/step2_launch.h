// Arguments of the on-chip-z kernels (k_fused.h), filled in one place for api_step2_cov / _apply / _istft.hip
#pragma once
#include "host.h"
#include "k_fused.h"

namespace disco_host {
// the cov kernel takes mask, z_out, part, chunks; the apply kernels w_glo, yf (and chunks); what a kernel does not read is NULL
inline disco::Step2Args step2_args(const disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* w_loc, const disco_c32* w_glo,
                                   disco_c32* z_out, disco_c32* yf, float4* part, int chunks) {
    disco::Step2Args a;
    a.X = (const disco::c32*)X;
    a.mask = mask;
    a.w_loc = (const disco::c32*)w_loc;
    a.w_glo = (const disco::c32*)w_glo;
    a.z_out = (disco::c32*)z_out;
    a.yf = (disco::c32*)yf;
    a.part = part;
    a.K = ctx->cfg.nodes;
    a.T = ctx->T;
    a.F = ctx->F;
    a.chunks = chunks;
    a.lens = ctx->d_lens;
    return a;
}
}  // namespace disco_host
