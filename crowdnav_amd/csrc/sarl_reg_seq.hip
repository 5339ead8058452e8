// The register-resident kernels of cadrl.ValueNetwork and the two lstm_rl networks (sarl_reg_seq_kernel.h) and their launcher
// (sarl_host.h); their weight streams are allocated and packed by sarl_reg.hip.
#include "sarl_host.h"
#include "sarl_reg_seq_kernel.h"

namespace {

int launch_reg_cadrl(cn_engine* e, const SarlPass& pass) {
    const cn_sarl* s = e->sarl;
    const int NT = s->cadrl_nt;  // (CADRL keeps fewer activations alive than SARL: 4 / 2 waves per SIMD at 1 / 2 humans per chunk)
    const bool ok = pick_int<1, 2, 3, 4, 5>(NT, [&](auto nt) {
        hipLaunchKernelGGL(cn::cadrl_reg_kernel<decltype(nt)::value>, reg_grid(s, pass, NT == 1 ? 4u : NT == 2 ? 2u : 1u), kRegBlock, 0,
                           e->stream, s->reg_stream, s->X, s->V, (int)pass.n_groups, (int)pass.n_tiles, s->net.ks_x, s->hcount, s->C.H,
                           s->cadrl_chunks);
    });
    return ok ? CN_OK : bad_humans(s->C.H);
}

void launch_reg_lstm(cn_engine* e, const SarlPass& pass) {  // RegLstm, RegLstm2: 4 or 16 input k-steps
    const cn_sarl* s = e->sarl;
    pick_bool(s->net.in_dim != 13, [&](auto wide) {
        constexpr int KS = decltype(wide)::value ? 16 : 4;
        if (s->route == SarlRoute::RegLstm2)
            hipLaunchKernelGGL(cn::lstm2_reg_kernel<KS>, reg_grid(s, pass, 1), kRegBlock, 0, e->stream, s->reg_stream, s->reg_stream3,
                               s->reg_stream2, s->X, s->V, (int)pass.n_groups, (int)pass.n_tiles, s->C.H, s->net.ks_x, s->hcount);
        else
            hipLaunchKernelGGL(cn::lstm_reg_kernel<KS>, reg_grid(s, pass, 1), kRegBlock, 0, e->stream, s->reg_stream, s->reg_stream2, s->X,
                               s->V, (int)pass.n_groups, (int)pass.n_tiles, s->C.H, s->net.ks_x, s->hcount);
    });
}

}  // namespace

int launch_reg_seq(cn_engine* e, const SarlPass& pass) {
    if (e->sarl->route == SarlRoute::RegCadrl) return launch_reg_cadrl(e, pass);
    launch_reg_lstm(e, pass);
    return CN_OK;
}
