// sarl_reg_chunk_kernel (sarl.ValueNetwork in registers for more than 5 humans) and its launcher (sarl_host.h); its three weight
// streams are allocated and packed by sarl_reg.hip.  A unit of its own: compiled beside cadrl_reg_kernel and lstm2_reg_kernel,
// hipcc gives those another instruction stream.
#include "sarl_host.h"
#include "sarl_reg_chunk_kernel.h"

int launch_reg_chunk(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;  // (launch_reg has launched the occupancy-map term where the stream starts from it)
    const bool ok = pick_int<3, 4>(s->chunk_nt, [&](auto nt) {
        pick_bool(s->pre, [&](auto pre) {
            pick_bool(att != nullptr, [&](auto a) {
                hipLaunchKernelGGL((cn::sarl_reg_chunk_kernel<decltype(nt)::value, decltype(pre)::value, decltype(a)::value>),
                                   reg_grid(s, pass, 1), kRegBlock, 0, e->stream, s->reg_stream, s->reg_stream3, s->reg_stream2, s->X, s->V,
                                   s->reg_scratch, (int)pass.n_groups, (int)pass.n_tiles, s->C.H, s->n_chunks, s->net.ks_x, s->hcount,
                                   (const float*)s->om_term, s->C.n_actions, att);
            });
        });
    });
    return ok ? CN_OK : bad_humans(s->C.H);
}
