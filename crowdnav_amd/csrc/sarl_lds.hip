// The value network with a tile's activations in LDS (sarl_lds_kernels.h): the sizes of its buffers and its launcher
// (sarl_host.h).  Its weights are the packed layers every configuration uploads (sarl_abi.hip).
#include "sarl_host.h"
#include "sarl_lds_kernels.h"

void sarl_lds_size(cn_sarl* s, bool* lds_chunked) {
    const cn_sarl_config* c = &s->cfg;
    cn::SarlNet& net = s->net;
    const bool cadrl = is_cadrl(*c), lstm = is_lstm(*c), pairwise = is_pairwise(*c);
    const int H = s->C.H, in_dim = net.in_dim;
    const int m1a = c->mlp1_dims[0], m1b = c->mlp1_dims[1], m2a = c->mlp2_dims[0], m2b = c->mlp2_dims[1];
    const int a0 = c->attention_dims[0], a1 = c->attention_dims[1];
    const int j0 = c->mlp3_dims[0], j1 = c->mlp3_dims[1], j2 = c->mlp3_dims[2];
    const int hid = c->mlp1_dims[0];  // LSTM-RL: hidden width
    auto max2 = [](int a, int b) { return a > b ? a : b; };
    // k-steps per row tile of each LDS buffer = whole column tiles of the widest layer written into it
    auto ks_of = [](int n) { return cn::sarl_ks(n); };
    bool& chunked = *lds_chunked;
    net.ks_x = ks_of(in_dim);
    net.ks_a = ks_of(max2(max2(max2(m1a, m2a), max2(a0, 6 + m2b)), max2(max2(j0, j1), j2)));
    net.ks_b = max2(ks_of(max2(m1b, a1)), net.ks_x);
    net.ks_c = ks_of(m2b);
    net.ks_s = 4;
    if (lstm) {
        net.ks_a = ks_of(max2(max2(j0, j1), max2(j2, 6 + hid)));
        net.ks_b = net.ks_c = 0;
        if (pairwise) {  // ping-pong buffers of ValueNetwork2.mlp1, all H row tiles: widths d0, d2 -> ks_b; d1, d3 -> ks_c
            const int* id = c->interaction_dims;
            net.ks_b = ks_of(max2(id[0], id[2]));
            net.ks_c = ks_of(max2(id[1], id[3]));
        }
        // more than kSarlMaxHumans humans: lstm_mlp_anyh_kernel stages one human's row tile per LSTM step (nothing sized by H)
        // (... and whenever H row tiles do not fit: ValueNetwork2's ping-pong buffers from 6 humans on)
        chunked = H > cn::kSarlMaxHumans || cn::lstm_lds_bytes(net, H, hid) > 160 * 1024;
        s->lds_bytes = cn::lstm_lds_bytes(net, chunked ? 1 : H, hid);
    } else if (cadrl) {  // ping-pong between A (first / third hidden layer) and B (X staging, second hidden layer)
        net.ks_a = ks_of(max2(j0, j2));
        net.ks_b = max2(ks_of(j1), net.ks_x);
        net.ks_c = 0;
        chunked = H > cn::kSarlMaxHumans;  // cadrl_mlp_chunked_kernel streams the humans in chunks of 5
        s->lds_bytes = cn::cadrl_lds_bytes(net, chunked ? cn::kSarlChunk : H, chunked);
    } else {
        // one tile's activations + the side chain's pong buffer (sarl_mlp_pipe_kernel) in LDS, or the humans stream through
        // in chunks (6+ humans at the shipped widths)
        s->pipe_lds_bytes = cn::sarl_pipe_lds_bytes(net, H);
        chunked = H > cn::kSarlMaxHumans || s->pipe_lds_bytes > 160 * 1024;
        s->lds_bytes = chunked ? cn::sarl_chunked_lds_bytes(net) : s->pipe_lds_bytes;
    }
}

int launch_lds(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;
    const dim3 grid((unsigned)pass.n_tiles), block(cn::kSarlThreads);
    const dim3 pgrid((unsigned)(pass.n_tiles < (size_t)s->n_cus ? pass.n_tiles : (size_t)s->n_cus));  // persistent: one workgroup per CU
    const int ng = (int)pass.n_groups;
    const bool cadrl = is_cadrl(s->cfg), lstm = is_lstm(s->cfg), chunked = s->route == SarlRoute::LdsChunked;
    if (chunked && cadrl)
        hipLaunchKernelGGL(cn::cadrl_mlp_chunked_kernel<cn::kSarlChunk>, grid, block, s->lds_bytes, e->stream, s->net, s->X, s->V, ng);
    else if (chunked && lstm)
        hipLaunchKernelGGL(cn::lstm_mlp_anyh_kernel, grid, block, s->lds_bytes, e->stream, s->net, s->X, s->V, ng);
    else if (chunked)
        pick_bool(att != nullptr, [&](auto a) {
            hipLaunchKernelGGL((cn::sarl_mlp_chunked_kernel<cn::kSarlChunk, decltype(a)::value>), grid, block, s->lds_bytes, e->stream,
                               s->net, s->X, s->V, ng, att);
        });
    if (chunked) return CN_OK;
    const bool ok = pick_int<1, 2, 3, 4, 5, 6, 7, 8>(s->C.H, [&](auto h) {
        constexpr int H = decltype(h)::value;
        if (cadrl)
            hipLaunchKernelGGL(cn::cadrl_mlp_kernel<H>, grid, block, s->lds_bytes, e->stream, s->net, s->X, s->V, ng, s->hcount);
        else if (lstm)
            hipLaunchKernelGGL(cn::lstm_mlp_kernel<H>, grid, block, s->lds_bytes, e->stream, s->net, s->X, s->V, ng, s->hcount);
        else
            pick_bool(att != nullptr, [&](auto a) {
                hipLaunchKernelGGL((cn::sarl_mlp_pipe_kernel<H, decltype(a)::value>), pgrid, block, s->lds_bytes, e->stream, s->ref,
                                   s->X, s->V, ng, (int)pass.n_tiles, s->hcount, att);
            });
    });
    return ok ? CN_OK : bad_humans(s->C.H);
}
