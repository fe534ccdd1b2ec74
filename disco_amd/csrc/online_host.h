// Host-side pieces of the online mode shared by its translation units (api_online.hip, api_online_ref.hip)
#pragma once
#include "host.h"
#include "k_online.h"

namespace disco_host {
// frames: the walk of this call (see OnlineArgs): T frames, planes of Tx (X, from frame tx0) / Tm (Z, mask, out) frames; state / init / phase:
// the resumable recursion of the streaming form (NULL / 0 / 0: a whole clip from Rss = 0, Rnn = init_diag I)
struct OnlineWalk {
    int T, Tx, tx0, Tm;
    c32* state;
    int init, phase;
};
// the argument rules of disco_online_mwf, stated once: 0 with *args filled for the walk wk, else the refusal of `who` (nothing is launched)
int online_args(disco_ctx* ctx, const char* who, const disco_c32* X, const disco_c32* Z, const float* mask, int P, float lambda_cor, float mu,
                int update_every, float init_diag, disco_c32* out, disco_c32* w_last, const OnlineWalk& wk, disco::OnlineArgs* args);
}  // namespace disco_host
