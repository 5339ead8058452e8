// The value network with the activations in registers (sarl_reg_kernel.h): the weight streams of its five routes and their
// packing, the hoisted occupancy-map term, and the launcher of sarl_reg_kernel (sarl_host.h).  The kernels of the other four
// routes are sarl_reg_chunk.hip's and sarl_reg_seq.hip's, which launch them on the streams packed here.
#include "sarl_host.h"
#include "sarl_reg_kernel.h"

namespace {

int sarl_alloc_stream(cn_engine* e, float** stream, int key) {
    return dev_alloc(e, stream, (size_t)cn::reg_total_quads(key) * 256);
}

// a layer of a register-resident kernel's weight stream: state_dict layer sd with the shape of packed layer kl
void reg_fill(const cn_sarl* s, cn::RegPackLayer& R, const float* const* p, int sd, int kl, int replicate = 0) {
    const cn::PackedLinear& L = s->net.L[kl];
    R.W = p[2 * sd], R.b = p[2 * sd + 1], R.N = L.N, R.K = L.K, R.ldw = L.K, R.k_off = 0, R.replicate = replicate;
}
void reg_pack(cn_engine* e, const cn::RegPackPlan& plan, float* stream) {
    const int total = cn::reg_total_quads(plan.xks) * 256;
    hipLaunchKernelGGL(cn::sarl_reg_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, e->stream, plan, stream);
}

constexpr int kHeadLayers[4] = {cn::kL_mlp3_0, cn::kL_mlp3_2, cn::kL_mlp3_4, cn::kL_mlp3_6};

// RegLstm / RegLstm2: the gate layer's stream (p: lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0), in front of it
// mlp1's (RegLstm2; m1: its four layers), then the value head's
void lstm_reg_pack(cn_engine* e, const float* const* m1p, const float* const* p, const cn::RegPackPlan& head) {
    const cn_sarl* s = e->sarl;
    cn::RegPackPlan gates{};
    gates.xks = s->stream_key;
    cn::RegPackLayer& G = gates.L[0];
    G.W = p[0], G.W2 = p[1], G.b = p[2], G.b2 = p[3];
    G.N = 4 * cn::kRegLstmHid, G.K = s->net.in_dim, G.ldw = s->net.in_dim, G.k_split = s->stream_key - cn::kRegLstmGates;
    float* gate_stream = s->reg_stream;
    if (s->route == SarlRoute::RegLstm2) {  // mlp1's stream, the gates on mlp1's 50 outputs
        const int kl[4] = {cn::kL_mlp2_0, cn::kL_mlp2_2, cn::kL_att_2, cn::kL_att_4};
        cn::RegPackPlan m1{};
        m1.xks = s->stream_key;
        for (int l = 0; l < 4; ++l) reg_fill(s, m1.L[l], m1p, l, kl[l]);
        reg_pack(e, m1, s->reg_stream);
        gates.xks = cn::kRegLstmGates + cn::kRegLstmKs;
        G.K = cn::kRegLstmHid, G.ldw = cn::kRegLstmHid, G.k_split = cn::kRegLstmKs;
        gate_stream = s->reg_stream3;
    }
    reg_pack(e, gates, gate_stream);
    reg_pack(e, head, s->reg_stream2);
}

// RegCadrl, RegLstm, RegLstm2.  state_dict order: [ValueNetwork2: mlp1.{0,2,4,6}] the value head's four layers [lstm.*]
void head_reg_pack(cn_engine* e, const float* const* params) {
    const cn_sarl* s = e->sarl;
    const float* const* p = is_pairwise(s->cfg) ? params + 8 : params;
    cn::RegPackPlan head{};  // the value head's parameters as a weight stream of cadrl_reg_kernel / lstm_reg_kernel / lstm2_reg_kernel
    head.xks = s->route == SarlRoute::RegCadrl ? s->stream_key : cn::kRegLstmHead;
    for (int l = 0; l < 4; ++l) reg_fill(s, head.L[l], p, l, kHeadLayers[l], l == 3 ? 1 : 0);
    if (s->route == SarlRoute::RegCadrl) reg_pack(e, head, s->reg_stream);
    else lstm_reg_pack(e, params, p + 8, head);
}

// RegSarl: the same parameters as the weight stream of sarl_reg_kernel; RegSarlChunk: the same 12 layers dealt over the three
// streams A, B, G of sarl_reg_chunk_kernel
void sarl_reg_pack_streams(cn_engine* e, const float* const* p) {
    const cn_sarl* s = e->sarl;
    const int sd[cn::kRegLayers] = {0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 9, 10};  // state_dict layer of each stream layer
    const int kl[cn::kRegLayers] = {cn::kL_mlp1_0, cn::kL_mlp1_2, cn::kL_mlp2_0, cn::kL_mlp2_2, cn::kL_att0_global, cn::kL_att0_local,
                                    cn::kL_att_2,  cn::kL_att_4,  cn::kL_mlp3_0, cn::kL_mlp3_2, cn::kL_mlp3_4,      cn::kL_mlp3_6};
    const int at[cn::kRegLayers][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 1}, {2, 0}, {1, 2}, {1, 3}, {1, 4}, {2, 1}, {2, 2}, {2, 3}, {2, 4}};  // chunk: {A B G, slot}
    const bool chunk = s->route == SarlRoute::RegSarlChunk;
    cn::RegPackPlan plan[3] = {};
    plan[0].xks = s->stream_key, plan[1].xks = cn::kRegChunkB, plan[2].xks = cn::kRegChunkG;
    for (int l = 0; l < cn::kRegLayers; ++l) {
        cn::RegPackLayer& R = chunk ? plan[at[l][0]].L[at[l][1]] : plan[0].L[l];
        reg_fill(s, R, p, sd[l], kl[l], l == cn::kR_att_4 || (chunk && l == cn::kR_mlp3_6) ? 1 : 0);
        if (l == cn::kR_mlp1_0 && s->pre) R.K = 13;  // the map columns live in om_w
        if (l == cn::kR_att0_local || l == cn::kR_att0_global) R.ldw = 2 * R.K;  // attention.0 sees [h2 | mean]
        if (l == cn::kR_att0_local) R.b = nullptr;
        if (l == cn::kR_att0_global) R.k_off = R.K;
    }
    reg_pack(e, plan[0], s->reg_stream);
    if (chunk) reg_pack(e, plan[2], s->reg_stream2), reg_pack(e, plan[1], s->reg_stream3);
}

void launch_om_term(cn_engine* e) {  // PRE: the occupancy-map half of mlp1.0, once per (env, human)
    const cn_sarl* s = e->sarl;
    const int rows = s->C.B * s->C.H;
    hipLaunchKernelGGL(cn::sarl_om_term_kernel, dim3((rows + cn::kOmTermRows - 1) / cn::kOmTermRows), dim3(cn::kOmTermThreads), 0,
                       e->stream, s->om_w, s->om, s->om_term, rows);
}

int launch_reg_sarl(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;
    const int H = s->C.H;
    // waves per SIMD by the kernels' register counts (of 512; scripts/kernel_resources.py): 1 / 2 humans 153 / 215 -> 3 / 2, which
    // also covers the dependent MFMA chain of the 1-human kernel
    const dim3 grid = reg_grid(s, pass, H == 1 ? 3u : H == 2 ? 2u : 1u);
    const bool ok = pick_int<1, 2, 3, 4, 5>(H, [&](auto nt) {
        pick_bool(s->pre, [&](auto pre) {
            pick_bool(att != nullptr, [&](auto a) {
                hipLaunchKernelGGL((cn::sarl_reg_kernel<4, decltype(nt)::value, decltype(pre)::value, decltype(a)::value>), grid,
                                   kRegBlock, 0, e->stream, s->reg_stream, s->X, s->V, (int)pass.n_groups, (int)pass.n_tiles, s->net.ks_x,
                                   s->hcount, (const float*)s->om_term, s->C.n_actions, att);
            });
        });
    });
    return ok ? CN_OK : bad_humans(H);
}

}  // namespace

int sarl_reg_alloc(cn_engine* e, cn_sarl* s) {
    const int H = s->C.H, ks_in = s->net.in_dim == 13 ? 4 : 16;
    int key2 = 0, key3 = 0;  // of reg_stream2, reg_stream3
    switch (s->route) {
        case SarlRoute::RegSarl: s->pre = s->net.in_dim != 13, s->stream_key = s->pre ? cn::kRegSarlPre : 4; break;
        case SarlRoute::RegSarlChunk:
            s->n_chunks = (H + 3) / 4, s->chunk_nt = (H + s->n_chunks - 1) / s->n_chunks;
            s->pre = s->net.in_dim != 13, s->stream_key = s->pre ? cn::kRegChunkAPre : cn::kRegChunkA;
            key2 = cn::kRegChunkG, key3 = cn::kRegChunkB;
            break;
        case SarlRoute::RegCadrl:
            s->stream_key = cn::kRegCadrl;
            s->cadrl_chunks = (H + cn::kRegHumans - 1) / cn::kRegHumans, s->cadrl_nt = (H + s->cadrl_chunks - 1) / s->cadrl_chunks;
            break;
        case SarlRoute::RegLstm: s->stream_key = cn::kRegLstmGates + ks_in, key2 = cn::kRegLstmHead; break;
        case SarlRoute::RegLstm2: s->stream_key = cn::kRegLstmMlp1 + ks_in, key2 = cn::kRegLstmHead, key3 = cn::kRegLstmGates + cn::kRegLstmKs; break;
        default: return CN_OK;
    }
    int rc;
    if ((rc = sarl_alloc_stream(e, &s->reg_stream, s->stream_key)) || (key2 && (rc = sarl_alloc_stream(e, &s->reg_stream2, key2))) ||
        (key3 && (rc = sarl_alloc_stream(e, &s->reg_stream3, key3))))
        return rc;
    if (s->route == SarlRoute::RegSarlChunk &&
        (rc = dev_alloc(e, &s->reg_scratch, (size_t)s->n_cus * cn::kRegWaves * s->n_chunks * s->chunk_nt * 7 * 256)))
        return rc;
    if (s->pre && ((rc = dev_alloc(e, &s->om_w, (size_t)160 * 49)) || (rc = dev_alloc(e, &s->om_term, (size_t)s->C.B * H * 160))))
        return rc;
    return CN_OK;
}

int sarl_reg_pack(cn_engine* e, const float* const* params) {
    const cn_sarl* s = e->sarl;
    if (s->route == SarlRoute::RegSarl || s->route == SarlRoute::RegSarlChunk) {
        sarl_reg_pack_streams(e, params);
        if (s->pre)  // mlp1.0's map columns and bias
            hipLaunchKernelGGL(cn::sarl_om_weights_kernel, dim3((160 * 49 + 255) / 256), dim3(256), 0, e->stream, params[0], params[1], s->om_w);
    } else if (s->route == SarlRoute::RegCadrl || s->route == SarlRoute::RegLstm || s->route == SarlRoute::RegLstm2) {
        head_reg_pack(e, params);
    }
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int launch_reg(cn_engine* e, const SarlPass& pass, float* att) {
    if (e->sarl->pre) launch_om_term(e);
    return e->sarl->route == SarlRoute::RegSarl ? launch_reg_sarl(e, pass, att) : launch_reg_chunk(e, pass, att);
}

#ifdef CN_PHASE_TIMING
int sarl_reg_cycles(unsigned long long* sum16, int reset) { return sarl_cycles_of(HIP_SYMBOL(cn::cn_sarl_cycles), sum16, reset); }
#endif
