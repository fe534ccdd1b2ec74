// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): library-owned device blocks and the record of
// the covariance partial sums held in them (struct Partials, host.h: the invariants are written there).  No kernel.
#include "host.h"

namespace disco_host {
int grow(disco_ctx* ctx, DevBlock& b, size_t need) {
    if (b.bytes >= need) return 0;
    if (b.p) {
        HIPCHK(ctx, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    HIPCHK(ctx, hipMalloc(&b.p, need));
    b.bytes = need;
    return 0;
}

int ensure_own_ws(disco_ctx* ctx, size_t bytes) {
    if (ctx->own_ws.bytes < bytes && ctx->ref_ws == ctx->own_ws.p) ctx->ref_ws = nullptr;
    return grow(ctx, ctx->own_ws, bytes);
}

void pending_drop(disco_ctx* ctx) {
    ctx->partials.pend_blocks = 0;
    ctx->partials.pend_tail = false;
}

static void step1_drop(disco_ctx* ctx) {
    ctx->partials.loc_M = 0;
    ctx->partials.loc_X = ctx->partials.loc_mask = nullptr;
}

void partials_forget(disco_ctx* ctx) {
    pending_drop(ctx);
    step1_drop(ctx);
}

// the full or the tail block, `bytes` large: a block that has to grow takes the records of its contents with it (host.h)
static float4* block_of(disco_ctx* ctx, size_t bytes, bool tail, int* rc) {
    Partials& ps = ctx->partials;
    DevBlock& b = tail ? ps.tail : ps.full;
    if (b.bytes < bytes) {
        if (!tail) partials_forget(ctx);
        else if (ps.pend_tail) pending_drop(ctx);
    }
    *rc = grow(ctx, b, bytes);
    return *rc ? nullptr : (float4*)b.p;
}

float4* partials_begin(disco_ctx* ctx, const SumsPlan& plan, int* rc) { return block_of(ctx, plan.bytes(ctx->F), plan.tail, rc); }

void partials_commit(disco_ctx* ctx, const SumsPlan& plan) {
    ctx->partials.pend_blocks = plan.blocks;
    ctx->partials.pend_P = plan.P;
    ctx->partials.pend_tail = plan.tail;
    if (!plan.tail) step1_drop(ctx);
}

void step1_keep(disco_ctx* ctx, const void* X, const void* mask) {
    Partials& ps = ctx->partials;
    ps.loc_M = ps.pend_P;
    ps.loc_blocks = ps.pend_blocks;
    ps.loc_X = X;
    ps.loc_mask = mask;
}

bool step1_any(const disco_ctx* ctx) { return ctx->partials.loc_M == ctx->cfg.mics; }

bool step1_held(const disco_ctx* ctx, const void* X, const void* mask) {
    return step1_any(ctx) && ctx->partials.loc_X == X && ctx->partials.loc_mask == mask;
}

bool partials_pending(const disco_ctx* ctx, PendingSums* out) {
    const Partials& ps = ctx->partials;
    if (ps.pend_blocks < 1) return false;
    out->part = (const float4*)(ps.pend_tail ? ps.tail.p : ps.full.p);
    out->blocks = ps.pend_blocks;
    out->P = ps.pend_P;
    out->part_loc = ps.pend_tail ? (const float4*)ps.full.p : nullptr;
    out->blocks_loc = ps.pend_tail ? ps.loc_blocks : 0;
    out->M_loc = ps.pend_tail ? ps.loc_M : 0;
    return true;
}

int partials_reserve(disco_ctx* ctx, size_t full_bytes, size_t tail_bytes) {
    int rc = 0;
    block_of(ctx, full_bytes, false, &rc);
    if (!rc) block_of(ctx, tail_bytes, true, &rc);
    return rc;
}

size_t partials_bytes(const disco_ctx* ctx) { return ctx->partials.full.bytes + ctx->partials.tail.bytes; }
}  // namespace disco_host
