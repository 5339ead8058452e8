// C ABI of the SARL robot decision (declared in include/crowdnav_amd.h): cn_sarl_* and the value-network kernels, a
// translation unit of its own (engine_host.h has what it shares with crowdnav_amd.hip).
#include "engine_host.h"
#include "sarl_kernels.h"
#include "sarl_lds_kernels.h"
#include "sarl_narrow_kernel.h"
#include "sarl_reg_kernel.h"
#include "sarl_f16_kernel.h"
#include "sarl_step_fused.h"

// The kernel family that runs the value network: chosen once per configuration (sarl_choose_route), then read by
// cn_sarl_set_weights (which weight streams to pack) and sarl_select (which launcher).  DESIGN.md §3.5 has the conditions.
enum class SarlRoute {
    LdsTile,       // sarl_mlp_pipe_kernel<H, ATT> / cadrl_mlp_kernel<H> / lstm_mlp_kernel<H>: a tile's activations in LDS
    LdsChunked,    // sarl_mlp_chunked_kernel<.., ATT> / cadrl_mlp_chunked_kernel / lstm_mlp_anyh_kernel: the humans do not fit one tile's LDS
    Narrow,        // sarl_narrow_kernel<LSTM, ATT>: a few decisions (train.py's single-episode sampling) on tiles of 16 / H groups, one per workgroup
    RegSarl, RegSarlChunk,        // activations in registers: sarl_reg_kernel<4, NT, PRE, ATT> (1..5 humans), sarl_reg_chunk_kernel<NT, PRE, ATT> (6+)
    RegCadrl, RegLstm, RegLstm2,  // cadrl_reg_kernel<NT>, lstm_reg_kernel<4 / 16>, lstm2_reg_kernel<4 / 16> (lstm_rl.ValueNetwork2)
    SplitF16,      // sarl_f16_kernel<XKB, NT, ATT>: CN_PRECISION_F16X2, activations in registers, split-f16 matrix instructions
};
// cn_sarl_network_route reports the route as CN_SARL_ROUTE_*: the same order
static_assert((int)SarlRoute::LdsTile == CN_SARL_ROUTE_LDS_TILE && (int)SarlRoute::LdsChunked == CN_SARL_ROUTE_LDS_CHUNKED &&
              (int)SarlRoute::Narrow == CN_SARL_ROUTE_NARROW && (int)SarlRoute::RegSarl == CN_SARL_ROUTE_REG_SARL &&
              (int)SarlRoute::RegSarlChunk == CN_SARL_ROUTE_REG_SARL_CHUNK && (int)SarlRoute::RegCadrl == CN_SARL_ROUTE_REG_CADRL &&
              (int)SarlRoute::RegLstm == CN_SARL_ROUTE_REG_LSTM && (int)SarlRoute::RegLstm2 == CN_SARL_ROUTE_REG_LSTM2 &&
              (int)SarlRoute::SplitF16 == CN_SARL_ROUTE_SPLIT_F16);

struct cn_sarl {
    cn_sarl_config cfg = {};
    cn::SarlCfg C = {};
    cn::SarlNet net = {};
    cn::SarlNetRef ref = {};        // the same layers as offsets into `arena` (persistent value-network kernel)
    float* arena = nullptr;         // one allocation for every layer's packed weights and biases
    size_t arena_used = 0;
    double* actions = nullptr;      // [K][2] device copy of the action table
    float* orca_vel = nullptr;      // [B][A][2]
    double* next_obs = nullptr;     // [B][H][5]
    float* om = nullptr;            // [B][H][cells*channels]
    double* reward = nullptr;       // [B][K]
    float* X = nullptr;             // [tiles][H][ks_x][64] (MFMA A-fragment order)
    float* V = nullptr;             // [B*K]
    int* hcount = nullptr;          // [tiles * 16] humans present per (env, action) group (num_humans unless the `mixed` rule parks some)
    size_t n_groups = 0, n_tiles = 0, lds_bytes = 0;  // lds_bytes: of the LDS kernel the configuration would run (LdsTile / LdsChunked)
    bool weights_set = false;
    SarlRoute route = SarlRoute::LdsTile;
    bool narrow() const { return route == SarlRoute::Narrow; }
    int stream_key = 0;             // key of reg_stream: 4 (13 features), kRegSarlPre, kRegChunkA / APre, kRegCadrl, kRegLstmGates / kRegLstmMlp1 + 4 / 16
    float* reg_stream = nullptr;    // register-resident routes: weight streams of reg_total_quads(key) quads of 256 floats
    float* reg_stream2 = nullptr;   // RegLstm / RegLstm2: the value head's stream, kRegLstmHead (reg_stream is the gate layer's / mlp1's)
    float* reg_stream3 = nullptr;   // RegLstm2: the gate layer's; RegSarlChunk: streams A, G, B = reg_stream, reg_stream2, reg_stream3
    float* reg_scratch = nullptr;   // RegSarlChunk: per-wave parking space for mlp1's output
    int chunk_nt = 0, n_chunks = 0;
    int cadrl_nt = 0, cadrl_chunks = 0;  // RegCadrl: humans per chunk (1..5), chunks per tile (1 up to 5 humans)
    bool pre = false;  // RegSarl / RegSarlChunk on 61 inputs: the 48 map cells' half of mlp1.0 is hoisted out of the action loop (sarl_om_term_kernel), X holds k-steps 0..3 only
    float* om_w = nullptr;          // mlp1.0's occupancy-map columns [48][160 slots] and its bias [160] (sarl_om_weights_kernel)
    float* om_term = nullptr;       // b + W[:, 13:61] om per (env, human), [B * H][160] in accumulator order
    int n_cus = 0;
    size_t narrow_tiles = 0, narrow_lds = 0;
    bool fused_step = false;        // cn_sarl_sample_step on the narrow route: decision + transition + next ORCA as one kernel (CROWDNAV_AMD_SARL_FUSED_STEP)
    _Float16* f16_stream = nullptr; // SplitF16: Wh / Wl of every (output tile, input block) in the order of use (sarl_f16_pack_kernel)
    float* f16_bias = nullptr;      // ... and the biases in accumulator order
    int* narrow_counter = nullptr;  // cn_sarl_sample_step: workgroups of sarl_narrow_kernel that have written their V
    double* narrow_value = nullptr; // ... and reward + gamma V per (env, action), each written by the tile that computed V
    float* state_rows = nullptr;    // cn_sarl_state_values on the narrow tiles: a pass's rows [n_groups][H][13] (allocated by the first call)
    cn::PackJobs pack_jobs = {};    // cn_sarl_set_weights: the layers to repack, run as one launch (sarl_pack_flush)
    int pack_blocks = 0;
};

void cn_sarl_release(cn_engine* e) {
    delete e->sarl;  // device buffers are owned by the engine's slabs
    e->sarl = nullptr;
}

namespace {

bool is_cadrl(const cn_sarl_config& c) { return c.model == CN_MODEL_CADRL; }
bool is_lstm(const cn_sarl_config& c) { return c.model == CN_MODEL_LSTM_RL; }
bool is_pairwise(const cn_sarl_config& c) { return is_lstm(c) && c.interaction_dims[0] > 0; }  // lstm_rl.ValueNetwork2
int om_width(const cn_sarl_config& c) { return c.with_om ? c.cell_num * c.cell_num * c.om_channel_size : 0; }

int sarl_validate(const cn_sarl_config* c, int H) {
    if (c->n_actions < 1) return fail(CN_ERR_INVALID, "n_actions must be >= 1");
    if (c->precision != CN_PRECISION_F32 && c->precision != CN_PRECISION_F16X2)
        return fail(CN_ERR_INVALID, "unknown precision %d (CN_PRECISION_F32 = 0, CN_PRECISION_F16X2 = 1)", c->precision);
    if (c->with_om && (c->cell_num < 1 || c->om_channel_size < 1 || c->om_channel_size > 3 || !(c->cell_size > 0)))
        return fail(CN_ERR_INVALID, "bad occupancy-map parameters");
    if (c->with_om && H < 2) return fail(CN_ERR_INVALID, "occupancy maps need at least 2 humans (multi_human_rl.py:117)");
    const bool cadrl = is_cadrl(*c), lstm = is_lstm(*c);
    if (c->model != CN_MODEL_SARL && !cadrl && !lstm)
        return fail(CN_ERR_INVALID, "unknown value-network model %d", c->model);
    if (cadrl && c->with_om) return fail(CN_ERR_INVALID, "CADRL has no occupancy-map input");
    if (cadrl && c->constant_velocity_model)
        return fail(CN_ERR_INVALID, "CADRL.predict always queries the env (cadrl.py:150): constant_velocity_model is for SARL / LSTM-RL");
    if (lstm && c->mlp1_dims[0] < 1) return fail(CN_ERR_INVALID, "LSTM-RL: mlp1_dims[0] must hold the hidden width");
    if (is_pairwise(*c))
        for (int i = 0; i < 4; ++i)
            if (c->interaction_dims[i] < 1) return fail(CN_ERR_INVALID, "LSTM-RL: interaction_dims needs 4 positive widths");
    if (!cadrl && !lstm) {
        for (int i = 0; i < 2; ++i)
            if (c->mlp1_dims[i] < 1 || c->mlp2_dims[i] < 1) return fail(CN_ERR_INVALID, "bad mlp dims");
        if (c->attention_dims[2] != 1) return fail(CN_ERR_UNSUPPORTED, "attention must end in a single output");
    }
    for (int i = 0; i < 3; ++i)
        if (c->mlp3_dims[i] < 1) return fail(CN_ERR_INVALID, "bad mlp dims");
    if (c->mlp3_dims[3] != 1) return fail(CN_ERR_UNSUPPORTED, "the value head must end in a single output");
    if (!cadrl && !lstm && (c->attention_dims[0] < 1 || c->attention_dims[1] < 1))
        return fail(CN_ERR_INVALID, "bad attention dims");
    return CN_OK;
}

constexpr size_t kSarlArenaFloats = (size_t)4 << 20;  // 16 MiB: the shipped networks pack into ~0.5 MiB

int sarl_alloc_layer(cn_sarl* s, cn::PackedLinear& L, int N, int K) {
    L.K = K, L.N = N, L.ksteps = (K + 3) / 4, L.ctiles = (N + 15) / 16;
    L.kpad = (L.ksteps + cn::kSarlKChunk - 1) / cn::kSarlKChunk * cn::kSarlKChunk;
    if (L.kpad > 255 || L.ctiles > 255) return fail(CN_ERR_UNSUPPORTED, "layer %d -> %d is wider than the packed descriptors hold", K, N);
    const size_t nw = (size_t)(L.ctiles * L.kpad + 2 * cn::kSarlKChunk) * 64, nb = ((size_t)L.ctiles * 16 + 63) / 64 * 64;
    if (s->arena_used + nw + nb > kSarlArenaFloats) return fail(CN_ERR_UNSUPPORTED, "value network does not fit the weight arena");
    L.w = s->arena + s->arena_used;
    L.bias = s->arena + s->arena_used + nw;
    s->arena_used += nw + nb;
    return CN_OK;
}

// The packed layers of the model, each with its place in the arena; the LDS buffers (k-steps per row tile), the bytes of the LDS
// kernel and the tile counts.  *lds_chunked: that kernel is the chunked one, the humans do not fit one tile's LDS.
int sarl_size_network(cn_sarl* s, bool* lds_chunked) {
    const cn_sarl_config* c = &s->cfg;
    cn::SarlNet& net = s->net;
    const bool cadrl = is_cadrl(*c), lstm = is_lstm(*c), pairwise = is_pairwise(*c);
    const int H = s->C.H, in_dim = net.in_dim;
    const int m1a = c->mlp1_dims[0], m1b = c->mlp1_dims[1], m2a = c->mlp2_dims[0], m2b = c->mlp2_dims[1];
    const int a0 = c->attention_dims[0], a1 = c->attention_dims[1];
    const int j0 = c->mlp3_dims[0], j1 = c->mlp3_dims[1], j2 = c->mlp3_dims[2];
    const int dims[cn::kSarlLayers][2] = {  // {N, K}
        {m1a, in_dim}, {m1b, m1a}, {m2a, m1b}, {m2b, m2a}, {a0, m1b}, {a0, m1b}, {a1, a0}, {1, a1},
        {j0, 6 + m2b}, {j1, j0}, {j2, j1}, {1, j2}};
    const int hid = c->mlp1_dims[0];  // LSTM-RL: hidden width
    for (int l = 0; l < cn::kSarlLayers; ++l) {
        net.L[l] = cn::PackedLinear{};
        int N = dims[l][0], K = dims[l][1];
        if (cadrl) {
            if (l < cn::kL_mlp3_0) continue;  // CADRL uses the value head only
            if (l == cn::kL_mlp3_0) K = in_dim;
        } else if (lstm) {  // weight_ih_l0, weight_hh_l0; ValueNetwork2.mlp1: 4 layers in the otherwise unused slots; the value head
            const int* id = c->interaction_dims;
            const int own[6][3] = {{cn::kL_mlp1_0, 4 * hid, pairwise ? id[3] : in_dim}, {cn::kL_mlp1_2, 4 * hid, hid}, {cn::kL_mlp2_0, id[0], in_dim},
                                   {cn::kL_mlp2_2, id[1], id[0]}, {cn::kL_att_2, id[2], id[1]}, {cn::kL_att_4, id[3], id[2]}};
            int k = 0;
            while (k < (pairwise ? 6 : 2) && own[k][0] != l) ++k;
            if (k < (pairwise ? 6 : 2)) N = own[k][1], K = own[k][2];
            else if (l < cn::kL_mlp3_0) continue;
            else if (l == cn::kL_mlp3_0) K = 6 + hid;
        }
        const int rc = sarl_alloc_layer(s, net.L[l], N, K);
        if (rc) return rc;
    }
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
        chunked = H > cn::kSarlMaxHumans || cn::sarl_pipe_lds_bytes(net, H) > 160 * 1024;
        s->lds_bytes = chunked ? cn::sarl_chunked_lds_bytes(net) : cn::sarl_pipe_lds_bytes(net, H);
    }
    s->n_groups = (size_t)s->C.B * s->C.n_actions;
    s->n_tiles = (s->n_groups + cn::kSarlGroups - 1) / cn::kSarlGroups;
    const size_t per_tile = (size_t)(cn::kSarlGroups / (H < 1 ? 1 : H));
    s->narrow_tiles = per_tile ? (s->n_groups + per_tile - 1) / per_tile : 0;
    s->narrow_lds = cn::sarl_narrow_lds_bytes(net, lstm);
    return CN_OK;
}

// the widths of the shipped networks (policy.config), which the register-resident kernels are compiled for
bool sarl_shipped_widths(const cn_sarl_config& c, int in_dim) {
    if (c.mlp3_dims[0] != 150 || c.mlp3_dims[1] != 100 || c.mlp3_dims[2] != 100) return false;
    if (is_cadrl(c)) return in_dim == 13;  // [cadrl] mlp_dims = 150, 100, 100, 1
    if (in_dim != 13 && in_dim != 61) return false;
    const int* id = c.interaction_dims;
    if (is_lstm(c))
        return c.mlp1_dims[0] == cn::kRegLstmHid &&
               (!is_pairwise(c) || (id[0] == 150 && id[1] == 100 && id[2] == 100 && id[3] == cn::kRegLstmHid));
    return c.with_global_state && c.mlp1_dims[0] == 150 && c.mlp1_dims[1] == 100 && c.mlp2_dims[0] == 100 && c.mlp2_dims[1] == 50 &&
           c.attention_dims[0] == 100 && c.attention_dims[1] == 100;
}

// CN_PRECISION_F16X2 is for what sarl_f16_kernel is compiled for; anything else is refused with its reason, never run in fp32
int sarl_f16_supported(const cn_engine* e, const cn_sarl_config& c, int H, int in_dim) {
    const char* why = is_cadrl(c)                     ? "CADRL has no split-f16 kernel (CN_MODEL_SARL only)"
                      : is_lstm(c)                    ? "LSTM-RL has no split-f16 kernel (CN_MODEL_SARL only)"
                      : !c.with_global_state          ? "with_global_state = 0 has no split-f16 kernel"
                      : !sarl_shipped_widths(c, in_dim) ? "the split-f16 kernel is compiled for the shipped layer widths (mlp1 150-100, mlp2 100-50, "
                                                        "attention 100-100-1, mlp3 150-100-100-1 on 13- or 61-wide rows)"
                      : H < 1 || H > cn::kRegHumans   ? "the split-f16 kernel holds the activations of 1..5 humans"
                      : e->cfg.scenario_rule == CN_MIXED ? "the split-f16 kernel does not run under the mixed rule"
                                                      : nullptr;
    return why ? fail(CN_ERR_UNSUPPORTED, "CN_PRECISION_F16X2: %s (%d humans)", why, H) : CN_OK;
}

SarlRoute sarl_route_f32(const cn_sarl* s, bool lds_chunked);
// THE route decision, from the validated and sized configuration (lds_chunked: sarl_size's answer).
SarlRoute sarl_choose_route(const cn_sarl* s, bool lds_chunked) {
    const SarlRoute r = sarl_route_f32(s, lds_chunked);
    // CN_PRECISION_F16X2 (sarl_f16_supported has passed) takes over the throughput routes; the narrow tiles are latency-bound and stay
    if (s->cfg.precision == CN_PRECISION_F16X2 && (r == SarlRoute::LdsTile || r == SarlRoute::RegSarl)) return SarlRoute::SplitF16;
    return r;
}
// ... of CN_PRECISION_F32
SarlRoute sarl_route_f32(const cn_sarl* s, bool lds_chunked) {
    const cn_sarl_config& c = s->cfg;
    const cn::SarlCfg& C = s->C;
    const cn::SarlNet& net = s->net;
    const int H = C.H, in_dim = net.in_dim;
    const bool cadrl = is_cadrl(c), lstm = is_lstm(c), pairwise = is_pairwise(c);
    // The register-resident kernels are compiled for the shipped networks.  They are THROUGHPUT kernels: one wave carries a tile
    // through the whole network in ~86 us, 1024 of them at a time; the LDS kernel puts a whole workgroup on a tile (37 us, 256 at
    // a time).  Up to 512 tiles (~100 envs x 81 actions: the single-episode sampling of train.py) the LDS kernel finishes first.
    // CROWDNAV_AMD_SARL_REG: 0 never, 1 (default) by size, 2 always.
    const int reg_mode = env_int("CROWDNAV_AMD_SARL_REG", 1);
    if (sarl_shipped_widths(c, in_dim) && (reg_mode == 2 || (reg_mode == 1 && s->n_tiles > 512))) {
        if (pairwise) return SarlRoute::RegLstm2;
        if (lstm) return SarlRoute::RegLstm;  // any number of humans
        if (H >= 1) return cadrl ? SarlRoute::RegCadrl : H <= cn::kRegHumans ? SarlRoute::RegSarl : SarlRoute::RegSarlChunk;
    }
    // Few decisions: 16-row tiles of whole groups, one per workgroup, X built in the kernel (sarl_narrow_kernel) — while the
    // whole launch is at most one workgroup per CU (measured, a sampled step of 5 humans x 81 actions: 8 envs 53 us against
    // 73 us on the one-tile kernels, 16 envs 90 against 74: 16-group tiles do ~1.5 x less matrix work per group).
    // CROWDNAV_AMD_SARL_NARROW: 0 never, 1 (default) by size, 2 whenever the configuration allows it.
    const int narrow_mode = env_int("CROWDNAV_AMD_SARL_NARROW", 1);
    // LSTM-RL (round 6): lstm_rl.ValueNetwork1 with the environment queried (the joint state LstmRL.predict sorted feeds the
    // network only under the constant-velocity model); its straight-line k loops hold W_ih rows of up to 80 inputs and W_hh
    // of up to 60 hidden units
    const bool lstm_ok = !lstm || (!pairwise && net.L[cn::kL_mlp1_0].kpad <= 4 * cn::kSarlKChunk &&
                                   net.L[cn::kL_mlp1_2].kpad <= 3 * cn::kSarlKChunk && net.L[cn::kL_mlp3_0].kpad <= cn::kNarrowK);
    if (lstm_ok && !lds_chunked && (in_dim == 13 || (C.with_om && !cadrl)) && !C.sort_lookahead && H >= 1 &&
        H <= cn::kSarlMaxHumans && s->narrow_lds <= 160 * 1024 &&
        (narrow_mode == 2 || (narrow_mode == 1 && s->narrow_tiles <= (size_t)s->n_cus)))
        return SarlRoute::Narrow;
    return lds_chunked ? SarlRoute::LdsChunked : SarlRoute::LdsTile;
}

int sarl_alloc_stream(cn_engine* e, float** stream, int key) {
    return dev_alloc(e, stream, (size_t)cn::reg_total_quads(key) * 256);
}

// what the register-resident routes need beside the common buffers: their weight streams
int sarl_alloc_route(cn_engine* e, cn_sarl* s) {
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
        case SarlRoute::SplitF16: {
            const int xkb = cn::f16_key(s->net.in_dim == 13 ? 1 : 2, H);
            int rc;
            if ((rc = dev_alloc(e, &s->f16_stream, cn::f16_stream_bytes(xkb) / sizeof(_Float16))) ||
                (rc = dev_alloc(e, &s->f16_bias, (size_t)cn::f16_total_tiles(xkb) * 256)))
                return rc;
            return CN_OK;
        }
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

// the packing jobs of one cn_sarl_set_weights call are collected and run as ONE launch (sarl_pack_flush)
int sarl_pack_flush(cn_engine* e) {
    cn::PackJobs& jobs = e->sarl->pack_jobs;
    if (jobs.n > 0) {
        hipLaunchKernelGGL(cn::sarl_pack_many_kernel, dim3((unsigned)e->sarl->pack_blocks), dim3(256), 0, e->stream, jobs);
        jobs.n = 0, e->sarl->pack_blocks = 0;
        CN_HIP(hipGetLastError());
    }
    return CN_OK;
}
// columns k_off .. k_off + L.K of W [N][K] (and bias, or nullptr) into packed layer L
int sarl_pack(cn_engine* e, cn::PackedLinear& L, const float* W, const float* bias, int N, int K, int k_off) {
    cn::PackJobs& jobs = e->sarl->pack_jobs;
    if (jobs.n == cn::kPackJobs) {
        const int rc = sarl_pack_flush(e);
        if (rc) return rc;
    }
    const int total = L.ctiles * L.kpad * 64;
    cn::PackJob& J = jobs.job[jobs.n++];
    J.W = W, J.bias = bias, J.wp = const_cast<float*>(L.w), J.bp = const_cast<float*>(L.bias);
    J.N = N, J.K = K, J.k_offset = k_off, J.k_count = L.K, J.kpad = L.kpad, J.ctiles = L.ctiles, J.first_block = e->sarl->pack_blocks;
    e->sarl->pack_blocks += (total + 255) / 256;
    return CN_OK;
}
// parameters 2 sd, 2 sd + 1 of the state_dict (W, b) into the whole of packed layer kl
int sarl_pack_whole(cn_engine* e, const float* const* p, int sd, int kl) {
    cn::PackedLinear& L = e->sarl->net.L[kl];
    return sarl_pack(e, L, p[2 * sd], p[2 * sd + 1], L.N, L.K, 0);
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

// CADRL and LSTM-RL.  state_dict order: [ValueNetwork2: mlp1.{0,2,4,6}] the value head's four layers [lstm.*]
int sarl_set_weights_head(cn_engine* e, const float* const* params) {
    cn_sarl* s = e->sarl;
    int rc;
    const float* const* p = params;
    if (is_pairwise(s->cfg)) {
        const int kl[4] = {cn::kL_mlp2_0, cn::kL_mlp2_2, cn::kL_att_2, cn::kL_att_4};
        for (int i = 0; i < 4; ++i)
            if ((rc = sarl_pack_whole(e, p, i, kl[i]))) return rc;
        p += 8;
    }
    for (int i = 0; i < 4; ++i)
        if ((rc = sarl_pack_whole(e, p, i, kHeadLayers[i]))) return rc;
    cn::RegPackPlan head{};  // the same parameters as a weight stream of cadrl_reg_kernel / lstm_reg_kernel / lstm2_reg_kernel
    head.xks = s->route == SarlRoute::RegCadrl ? s->stream_key : cn::kRegLstmHead;
    for (int l = 0; l < 4; ++l) reg_fill(s, head.L[l], p, l, kHeadLayers[l], l == 3 ? 1 : 0);
    if (s->route == SarlRoute::RegCadrl) reg_pack(e, head, s->reg_stream);
    if (is_lstm(s->cfg)) {  // lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0
        cn::PackedLinear& Li = s->net.L[cn::kL_mlp1_0];
        cn::PackedLinear& Lh = s->net.L[cn::kL_mlp1_2];
        if ((rc = sarl_pack(e, Li, p[8], p[10], Li.N, Li.K, 0)) || (rc = sarl_pack(e, Lh, p[9], p[11], Lh.N, Lh.K, 0))) return rc;
    }
    if (s->route == SarlRoute::RegLstm || s->route == SarlRoute::RegLstm2) lstm_reg_pack(e, params, p + 8, head);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// RegSarl: the same parameters as the weight stream of sarl_reg_kernel; RegSarlChunk: the same 12 layers dealt over the three
// streams A, B, G of sarl_reg_chunk_kernel
void sarl_reg_pack(cn_engine* e, const float* const* p) {
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

// SARL.  state_dict layer i -> packed layer(s)
int sarl_set_weights_sarl(cn_engine* e, const float* const* p) {
    cn_sarl* s = e->sarl;
    cn::SarlNet& net = s->net;
    int rc;
    const int map[11] = {cn::kL_mlp1_0, cn::kL_mlp1_2, cn::kL_mlp2_0, cn::kL_mlp2_2, cn::kL_att0_local, cn::kL_att_2,
                         cn::kL_att_4,  cn::kL_mlp3_0, cn::kL_mlp3_2, cn::kL_mlp3_4, cn::kL_mlp3_6};
    for (int i = 0; i < 11; ++i) {
        if (map[i] != cn::kL_att0_local) {
            if ((rc = sarl_pack_whole(e, p, i, map[i]))) return rc;
            continue;
        }
        cn::PackedLinear& L = net.L[map[i]];
        const int half = L.K;  // mlp1 output width
        const int Ktot = net.with_global ? 2 * half : half;
        if ((rc = sarl_pack(e, L, p[2 * i], p[2 * i + 1], L.N, Ktot, 0))) return rc;
        if (net.with_global && (rc = sarl_pack(e, net.L[cn::kL_att0_global], p[2 * i], nullptr, L.N, Ktot, half))) return rc;
    }
    if (s->route == SarlRoute::SplitF16) {  // Wh / Wl in the matrix instruction's operand order, the biases in accumulator order: one launch
        cn::F16PackPlan plan{};
        plan.xkb = cn::f16_key(net.in_dim == 13 ? 1 : 2, s->C.H);
        for (int l = 0; l < 11; ++l) plan.W[l] = p[2 * l], plan.b[l] = p[2 * l + 1];
        const int total = cn::f16_total_items(plan.xkb) * 512 + cn::f16_total_tiles(plan.xkb) * 256;
        hipLaunchKernelGGL(cn::sarl_f16_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, e->stream, plan, s->f16_stream, s->f16_bias);
        CN_HIP(hipGetLastError());
    }
    if (s->route != SarlRoute::RegSarl && s->route != SarlRoute::RegSarlChunk) return CN_OK;
    sarl_reg_pack(e, p);
    if (s->pre)  // mlp1.0's map columns and bias
        hipLaunchKernelGGL(cn::sarl_om_weights_kernel, dim3((160 * 49 + 255) / 256), dim3(256), 0, e->stream, p[0], p[1], s->om_w);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// the humans' next states and the occupancy map each of them sees: once per (env, human)
void launch_lookahead(cn_engine* e) {
    const cn_sarl* s = e->sarl;
    hipLaunchKernelGGL(cn::sarl_lookahead_kernel, dim3((s->C.B * s->C.H + 255) / 256), dim3(256), 0, e->stream, s->C, e->S.pos, e->S.vel,
                       e->S.rv, s->orca_vel, s->next_obs, s->om);
}

// X of every (env, action, human); om_columns = 0: k-steps 0..3 only; orca_vel == nullptr: the humans' next states from next_obs
void launch_features(cn_engine* e, int om_columns, const float* orca_vel) {
    const cn_sarl* s = e->sarl;
    const size_t rows = s->n_tiles * cn::kSarlGroups * s->C.H;
    hipLaunchKernelGGL(cn::sarl_feature_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream, s->C, s->net.in_dim,
                       s->net.ks_x, e->S.pos, e->S.goal, e->S.rv, e->S.theta, s->actions, s->next_obs, s->om, s->X, s->n_tiles,
                       s->hcount, om_columns, e->S.vel, orca_vel);
}

// Narrow: `tiles` workgroups write V; om: the occupancy maps or nullptr; att != nullptr (SARL): the ATT instantiation
void launch_narrow(cn_engine* e, unsigned tiles, const cn::SarlDecide& D, float* V, const float* om, float* att) {
    const cn_sarl* s = e->sarl;
    const auto narrow_kernel = is_lstm(s->cfg) ? cn::sarl_narrow_kernel<true>
                               : att           ? cn::sarl_narrow_kernel<false, true>
                                               : cn::sarl_narrow_kernel<false>;
    hipLaunchKernelGGL(narrow_kernel, dim3(tiles), dim3(cn::kNarrowThreads), s->narrow_lds, e->stream, s->ref, s->C, e->S.pos, e->S.vel,
                       e->S.goal, e->S.rv, e->S.theta, s->actions, s->orca_vel, s->next_obs, V, D, om, att);
    e->launch_counts[CN_COUNT_SARL_NARROW] += 1;
}

// What one launch of the network kernels evaluates: the first n_groups groups of X / hcount / V, on n_tiles tiles of kSarlGroups.
// A decision is the whole of the engine's buffers (whole_pass); cn_sarl_state_values fills them pass by pass, the last one shorter.
struct SarlPass {
    size_t n_groups, n_tiles;
};
SarlPass whole_pass(const cn_sarl* s) { return SarlPass{s->n_groups, s->n_tiles}; }
SarlPass pass_of(size_t groups) { return SarlPass{groups, (groups + cn::kSarlGroups - 1) / cn::kSarlGroups}; }

// the persistent grid of a register-resident kernel: a wave per tile, at most per_cu workgroups (= waves per SIMD) per CU
dim3 reg_grid(const cn_sarl* s, const SarlPass& pass, unsigned per_cu) {
    const unsigned wgs = (unsigned)((pass.n_tiles + cn::kRegWaves - 1) / cn::kRegWaves), resident = (unsigned)s->n_cus * per_cu;
    return dim3(wgs < resident ? wgs : resident);
}
const dim3 kRegBlock(cn::kRegWaves * 64);

int bad_humans(int H) { return fail(CN_ERR_UNSUPPORTED, "value network on device: %d humans", H); }

void launch_om_term(cn_engine* e) {  // PRE: the occupancy-map half of mlp1.0, once per (env, human)
    const cn_sarl* s = e->sarl;
    const int rows = s->C.B * s->C.H;
    hipLaunchKernelGGL(cn::sarl_om_term_kernel, dim3((rows + cn::kOmTermRows - 1) / cn::kOmTermRows), dim3(cn::kOmTermThreads), 0,
                       e->stream, s->om_w, s->om, s->om_term, rows);
}

int launch_reg_sarl(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;
    const int H = s->C.H;
    if (s->pre) launch_om_term(e);
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

int launch_split_f16(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;
    const int H = s->C.H;
    const dim3 grid = reg_grid(s, pass, 1);  // one wave per SIMD at every crowd size (more than 256 registers; scripts/kernel_resources.py)
    const bool ok = pick_int<1, 2, 3, 4, 5>(H, [&](auto nt) {
        pick_bool(s->net.in_dim != 13, [&](auto wide) {
            pick_bool(att != nullptr, [&](auto a) {
                hipLaunchKernelGGL((cn::sarl_f16_kernel<cn::f16_key(decltype(wide)::value ? 2 : 1, decltype(nt)::value), decltype(nt)::value, decltype(a)::value>), grid,
                                   kRegBlock, 0, e->stream, (const _Float16*)s->f16_stream, (const float*)s->f16_bias, (const float*)s->X,
                                   s->V, (int)pass.n_groups, (int)pass.n_tiles, s->net.ks_x, (const int*)s->hcount, att);
            });
        });
    });
    return ok ? CN_OK : bad_humans(H);
}

int launch_reg_sarl_chunk(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;
    if (s->pre) launch_om_term(e);
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

// LdsTile, LdsChunked — and the one-tile kernel of a configuration whose decisions take the narrow tiles (sarl_state_values)
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

// The network on the groups of `pass` as X / hcount hold them, V into s->V: the route's kernel; on a narrow-route engine (whose
// decisions never put X in HBM) the configuration's LDS one-tile kernel, whose packed layers every configuration uploads.
int launch_network(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;
    switch (s->route) {
        case SarlRoute::RegSarl: return launch_reg_sarl(e, pass, att);
        case SarlRoute::RegSarlChunk: return launch_reg_sarl_chunk(e, pass, att);
        case SarlRoute::SplitF16: return launch_split_f16(e, pass, att);
        case SarlRoute::RegCadrl: return launch_reg_cadrl(e, pass);
        case SarlRoute::RegLstm:
        case SarlRoute::RegLstm2: launch_reg_lstm(e, pass); return CN_OK;
        case SarlRoute::Narrow:
        case SarlRoute::LdsChunked:
        case SarlRoute::LdsTile: return launch_lds(e, pass, att);
    }
    return CN_OK;
}

// cn_sarl_select and cn_sarl_select_attention: att == nullptr launches exactly cn_sarl_select's kernels; otherwise every SARL
// route takes its ATT instantiation, which also writes the softmax weights it holds, float [B][n_actions][H]
int sarl_select(cn_engine* e, double* values, int32_t* best, double* action, float* att) {
    int rc = bind(e);
    if (rc) return rc;
    cn_sarl* s = e->sarl;
    if (!s || !s->weights_set) return fail(CN_ERR_INVALID, "cn_sarl_select: configure and set weights first");
    if (!best || !action) return fail(CN_ERR_INVALID, "cn_sarl_select: best/action must not be NULL");
    const cn::SarlCfg& C = s->C;
    // humans' next velocities, once per env (query_env = false: they keep their current ones, no ORCA pass)
    if (!C.const_vel) cn_launch_orca(e, s->orca_vel);
    // the humans' next observable states: their own kernel only where something is built on them per (env, human) — occupancy
    // maps, LSTM-RL's re-ordering; otherwise the feature kernel derives them itself.  The reward of every (env, action) is
    // evaluated inside sarl_select_kernel.  (Each small kernel less is ~7 us of a 70 us single-env decision.)
    const bool lookahead = C.with_om || C.sort_lookahead;
    if (lookahead) launch_lookahead(e);
    if (!s->narrow()) launch_features(e, s->pre ? 0 : 1, lookahead ? (const float*)nullptr : (const float*)s->orca_vel);
    if (s->narrow()) {  // X never leaves the network kernel's LDS
        cn::SarlDecide D0{};
        D0.in_dim = s->net.in_dim;
        launch_narrow(e, (unsigned)s->narrow_tiles, D0, s->V, C.with_om ? s->om : nullptr, att);
    } else if ((rc = launch_network(e, whole_pass(s), att))) {
        return rc;
    }
    hipLaunchKernelGGL(cn::sarl_select_kernel, dim3((C.B + 3) / 4), dim3(256), 0, e->stream, C, e->S.pos, e->S.vel, e->S.goal,
                       e->S.rv, e->S.gtime, e->S.theta, s->actions, s->reward, s->V, values, best, action);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// cn_sarl_state_values' conditions on the engine, which cn_lookahead_values shares (`who` speaks): INVALID before UNSUPPORTED
int state_values_check(const cn_engine* e, const char* who, bool have_theta) {
    const cn_sarl* s = e->sarl;
    if (!s || !s->weights_set) return fail(CN_ERR_INVALID, "%s: configure and set weights first", who);
    if (e->P.robot_unicycle && !have_theta)
        return fail(CN_ERR_INVALID, "%s: a CN_UNICYCLE engine needs the robot heading of every state (theta / out->final_theta is NULL)", who);
    if (s->cfg.with_om)
        return fail(CN_ERR_UNSUPPORTED, "%s: engines with occupancy maps (with_om) are not served: the maps of caller-held states "
                    "are not built on the device", who);
    if (e->cfg.scenario_rule == CN_MIXED)
        return fail(CN_ERR_UNSUPPORTED, "%s: engines under the mixed rule are not served: a caller-held state does not say which "
                    "humans are absent", who);
    return CN_OK;
}

// V of n caller-held joint states (state_values_check has passed): passes of at most n_groups states through the engine's X /
// hcount / V — or, where the narrow kernel takes caller rows, through state_rows and straight into `value`.
int state_values_run(cn_engine* e, const double* state8, const double* theta, int64_t n, int sort_humans, float* value) {
    cn_sarl* s = e->sarl;
    const int H = s->C.H;
    const bool rows_mode = s->narrow() && !is_cadrl(s->cfg);  // SarlDecide::x_rows, as cn_sarl_values; CADRL: the one-tile kernel
    int rc;
    if (rows_mode && !s->state_rows && (rc = dev_alloc(e, &s->state_rows, s->n_groups * H * 13))) return rc;  // the first call only
    for (size_t first = 0; first < (size_t)n; first += s->n_groups) {
        const size_t m = (size_t)n - first < s->n_groups ? (size_t)n - first : s->n_groups;
        const SarlPass pass = pass_of(m);
        const size_t lanes = pass.n_tiles * cn::kSarlGroups * H;
        hipLaunchKernelGGL(cn::sarl_state_feature_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream, H,
                           (int)e->P.robot_unicycle, sort_humans ? 1 : 0, state8, e->P.robot_unicycle ? theta : (const double*)nullptr,
                           first, m, pass.n_tiles, s->net.ks_x, s->X, s->hcount, rows_mode ? s->state_rows : (float*)nullptr);
        CN_HIP(hipGetLastError());
        if (rows_mode) {
            cn::SarlDecide D{};
            D.x_rows = s->state_rows, D.ext_groups = (int)m, D.in_dim = s->net.in_dim;
            const size_t GT = (size_t)(cn::kSarlGroups / H);
            launch_narrow(e, (unsigned)((m + GT - 1) / GT), D, value + first, nullptr, nullptr);
        } else {
            if ((rc = launch_network(e, pass, nullptr))) return rc;
            CN_HIP(hipMemcpyAsync(value + first, s->V, sizeof(float) * m, hipMemcpyDeviceToDevice, e->stream));
        }
        CN_HIP(hipGetLastError());
    }
    return CN_OK;
}

}  // namespace

extern "C" {

int cn_sarl_configure(cn_engine* e, const cn_sarl_config* c, const double* actions_host) {
    int rc = bind(e);
    if (rc) return rc;
    if (!c || !actions_host) return fail(CN_ERR_INVALID, "cn_sarl_configure: NULL argument");
    if (e->sarl) return fail(CN_ERR_INVALID, "cn_sarl_configure: already configured for this engine");
    const int H = e->cfg.num_humans;
    if ((rc = sarl_validate(c, H))) return rc;
    // built in a local object and handed to the engine only when everything below succeeded: a failed configure leaves
    // the engine unconfigured
    // ... and the device buffers allocated on the way are freed again: a host that retries configurations (say, falling
    // back from a chunked network under the mixed rule) must not leak the 16 MiB weight arena per attempt
    struct Guard {
        cn_sarl* p;
        cn_engine* e;
        cn_engine::AllocMark mark;
        ~Guard() {
            if (!p) return;  // success: ownership went to the engine
            e->alloc_rollback(mark);
            delete p;
        }
    } guard{new (std::nothrow) cn_sarl(), e, e->alloc_mark()};
    cn_sarl* s = guard.p;
    if (!s) return fail(CN_ERR_INVALID, "out of host memory");
    s->cfg = *c;
    {
        hipDeviceProp_t prop;
        CN_HIP(hipGetDeviceProperties(&prop, e->cfg.device));
        s->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    cn::SarlCfg& C = s->C;
    C.B = e->P.B, C.H = H, C.n_actions = c->n_actions;
    C.with_om = c->with_om ? 1 : 0, C.cell_num = c->cell_num, C.om_channels = c->om_channel_size, C.cell_size = c->cell_size;
    C.dt = e->P.dt, C.time_limit = e->P.time_limit, C.success_reward = e->P.success_reward;
    C.collision_penalty = e->P.collision_penalty, C.discomfort_dist = e->P.discomfort_dist;
    C.discomfort_factor = e->P.discomfort_factor;
    C.gamma_bar = std::pow(c->gamma, e->cfg.time_step * e->cfg.robot_v_pref);
    C.unicycle = e->P.robot_unicycle;
    C.const_vel = c->constant_velocity_model ? 1 : 0;
    C.cadrl = c->model == CN_MODEL_CADRL ? 1 : 0;
    C.sort_lookahead = (C.const_vel && c->model == CN_MODEL_LSTM_RL) ? 1 : 0;
    s->net.in_dim = 13 + om_width(*c), s->net.with_global = c->with_global_state ? 1 : 0, s->net.H = H;
    if (c->precision == CN_PRECISION_F16X2 && (rc = sarl_f16_supported(e, *c, H, s->net.in_dim))) return rc;
    bool lds_chunked = false;
    if ((rc = dev_alloc(e, &s->arena, kSarlArenaFloats)) || (rc = sarl_size_network(s, &lds_chunked))) return rc;
    s->route = sarl_choose_route(s, lds_chunked);
    s->fused_step = env_int("CROWDNAV_AMD_SARL_FUSED_STEP", 1) != 0 && e->P.threads == 64 && !e->P.kd;
    if ((rc = sarl_alloc_route(e, s))) return rc;
    if (s->lds_bytes > 160 * 1024)
        return fail(CN_ERR_UNSUPPORTED, "SARL network of this size needs %zu bytes of LDS per tile (> 160 KiB)", s->lds_bytes);
    if ((rc = dev_alloc(e, &s->actions, (size_t)2 * C.n_actions)) || (rc = dev_alloc(e, &s->orca_vel, (size_t)2 * C.B * (H + 1))) ||
        (rc = dev_alloc(e, &s->next_obs, (size_t)C.B * H * 5)) ||
        (rc = dev_alloc(e, &s->om, (size_t)C.B * H * (c->with_om ? om_width(*c) : 1))) ||
        (rc = dev_alloc(e, &s->reward, s->n_groups)) || (rc = dev_alloc(e, &s->V, s->n_tiles * cn::kSarlGroups)) ||
        (rc = dev_alloc(e, &s->X, s->n_tiles * H * s->net.ks_x * 64)) ||
        (rc = dev_alloc(e, &s->hcount, s->n_tiles * cn::kSarlGroups)) || (rc = dev_alloc(e, &s->narrow_counter, 1)) ||
        (rc = dev_alloc(e, &s->narrow_value, s->n_groups)))
        return rc;
    CN_HIP(hipMemset(s->narrow_counter, 0, sizeof(int)));
    if (e->cfg.scenario_rule == CN_MIXED && lds_chunked) {
        if (H <= cn::kSarlMaxHumans && c->model == CN_MODEL_SARL)  // the network, not the crowd, is too large for one tile
            return fail(CN_ERR_UNSUPPORTED,
                        "value networks under the mixed rule run the one-tile kernel (it masks an episode's absent humans), whose "
                        "tile — activations %zu B + the pipelined side buffer %zu B — must fit the 160 KiB of LDS; these layer "
                        "widths do not (narrower mlp1 / mlp3 layers do: the shipped 150-wide network needs 150.5 KiB)",
                        cn::sarl_pipe_lds_bytes(s->net, s->C.H) - sizeof(float) * 64 * (size_t)s->net.ks_a, sizeof(float) * 64 * (size_t)s->net.ks_a);
        return fail(CN_ERR_UNSUPPORTED,
                    "value networks under the mixed rule run the one-tile kernels (they mask an episode's absent humans): "
                    "num_humans must be 5 (the rule never draws more)");
    }
    CN_HIP(hipMemcpy(s->actions, actions_host, sizeof(double) * 2 * s->C.n_actions, hipMemcpyHostToDevice));
    const cn::SarlNet& net = s->net;
    cn::SarlNetRef& ref = s->ref;  // the same layers as offsets into the arena
    ref.base = s->arena;
    for (int l = 0; l < cn::kSarlLayers; ++l) {
        const cn::PackedLinear& L = net.L[l];
        if (!L.w) continue;
        ref.L[l] = cn::LayerRef{(uint32_t)(L.w - s->arena), (uint32_t)(L.bias - s->arena),
                                (uint32_t)L.kpad | ((uint32_t)L.ctiles << 8) | ((uint32_t)L.ksteps << 16)};
    }
    ref.nf = c->model == CN_MODEL_LSTM_RL ? c->mlp1_dims[0] : net.L[cn::kL_mlp2_2].N, ref.with_global = net.with_global;  // (LSTM-RL: the hidden width)
    ref.ks_x = net.ks_x, ref.ks_a = net.ks_a, ref.ks_b = net.ks_b, ref.ks_c = net.ks_c, ref.ks_s = net.ks_s;
    e->sarl = s;
    guard.p = nullptr;
    return CN_OK;
}

int cn_sarl_set_weights(cn_engine* e, const float* const* params_host_array) {
    int rc = bind(e);
    if (rc) return rc;
    cn_sarl* s = e->sarl;
    if (!s) return fail(CN_ERR_INVALID, "cn_sarl_set_weights: call cn_sarl_configure first");
    if (!params_host_array) return fail(CN_ERR_INVALID, "cn_sarl_set_weights: NULL");
    const bool cadrl = is_cadrl(s->cfg), lstm = is_lstm(s->cfg);
    s->pack_jobs.n = 0, s->pack_blocks = 0;  // (a call that failed half-way leaves nothing queued)
    for (int i = 0; i < (cadrl ? 8 : (lstm ? (is_pairwise(s->cfg) ? 20 : 12) : 22)); ++i)
        if (!params_host_array[i]) return fail(CN_ERR_INVALID, "cn_sarl_set_weights: parameter %d is NULL", i);
    // W0, b0, W1, b1, ... in state_dict order
    if ((rc = cadrl || lstm ? sarl_set_weights_head(e, params_host_array) : sarl_set_weights_sarl(e, params_host_array))) return rc;
    if ((rc = sarl_pack_flush(e))) return rc;
    s->weights_set = true;
    return CN_OK;
}

int cn_sarl_select(cn_engine* e, double* values, int32_t* best, double* action) {
    return sarl_select(e, values, best, action, nullptr);
}

int cn_sarl_select_attention(cn_engine* e, double* values, int32_t* best, double* action, float* attention) {
    if (attention) {
        int rc = bind(e);
        if (rc) return rc;
        const cn_sarl* s = e->sarl;
        if (!s) return fail(CN_ERR_INVALID, "cn_sarl_select_attention: configure and set weights first");
        if (s->cfg.model != CN_MODEL_SARL)
            return fail(CN_ERR_UNSUPPORTED, "cn_sarl_select_attention: only sarl.ValueNetwork has attention weights");
    }
    return sarl_select(e, values, best, action, attention);
}

int cn_sarl_network_route(cn_engine* e, int* route_host) {
    if (!e) return fail(CN_ERR_INVALID, "engine is NULL");
    if (!e->sarl) return fail(CN_ERR_INVALID, "cn_sarl_network_route: cn_sarl_configure first");
    if (!route_host) return fail(CN_ERR_INVALID, "cn_sarl_network_route: route_host is NULL");
    *route_host = (int)e->sarl->route;
    return CN_OK;
}

int cn_sarl_explore(cn_engine* e, double epsilon, const uint8_t* mask, int32_t* best, double* action,
                    uint8_t* explored) {
    int rc = bind(e);
    if (rc) return rc;
    cn_sarl* s = e->sarl;
    if (!s) return fail(CN_ERR_INVALID, "cn_sarl_explore: cn_sarl_configure first");
    if (!best || !action) return fail(CN_ERR_INVALID, "cn_sarl_explore: best/action must not be NULL");
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(CN_ERR_INVALID, "cn_sarl_explore: epsilon must be in [0, 1]");
    const cn::SarlCfg& C = s->C;
    hipLaunchKernelGGL(cn::sarl_explore_kernel, dim3((C.B + 63) / 64), dim3(64), 0, e->stream, C.B, C.n_actions, epsilon,
                       e->S.mt_key, e->S.mt_pos, s->actions, mask, best, action, explored, e->C.error);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_sarl_transform(cn_engine* e, float* out, int64_t env_stride, int sort_humans) {
    int rc = bind(e);
    if (rc) return rc;
    cn_sarl* s = e->sarl;
    if (!s) return fail(CN_ERR_INVALID, "cn_sarl_transform: cn_sarl_configure first");
    if (!out) return fail(CN_ERR_INVALID, "cn_sarl_transform: out is NULL");
    const cn::SarlCfg& C = s->C;
    const int64_t row = (int64_t)C.H * s->net.in_dim;
    if (env_stride == 0) env_stride = row;
    if (env_stride < row) return fail(CN_ERR_INVALID, "cn_sarl_transform: env_stride %lld < %lld", (long long)env_stride, (long long)row);
    hipLaunchKernelGGL(cn::sarl_transform_kernel, dim3((C.B * C.H + 255) / 256), dim3(256), 0, e->stream, C, s->net.in_dim,
                       sort_humans ? 1 : 0, e->S.pos, e->S.vel, e->S.goal, e->S.rv, e->S.theta, out, env_stride);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_sarl_sample_step(cn_engine* e, double epsilon, uint8_t* alive, int32_t* best, double* action, float* state_out,
                        int64_t env_stride, int sort_humans, double* reward, uint8_t* done, uint8_t* info, double* dmin) {
    const bool was_fresh = e && e->orca_fresh;  // bind() clears it: every entry point but this one invalidates the velocities
    int rc = bind(e);
    if (rc) return rc;
    cn_sarl* s = e->sarl;
    if (!s || !s->weights_set) return fail(CN_ERR_INVALID, "cn_sarl_sample_step: configure and set weights first");
    if (!alive || !best || !action || !reward || !done || !info)
        return fail(CN_ERR_INVALID, "cn_sarl_sample_step: alive, best, action, reward, done and info must not be NULL");
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(CN_ERR_INVALID, "cn_sarl_sample_step: epsilon must be in [0, 1]");
    if (e->P.robot_orca) return fail(CN_ERR_INVALID, "cn_sarl_sample_step: the robot must be CN_ROBOT_EXTERNAL");
    const cn::SarlCfg& C = s->C;
    const int64_t row = (int64_t)C.H * s->net.in_dim;
    if (env_stride == 0) env_stride = row;
    if (state_out && env_stride < row)
        return fail(CN_ERR_INVALID, "cn_sarl_sample_step: env_stride %lld < %lld", (long long)env_stride, (long long)row);
    const bool fresh = was_fresh;
    if (s->narrow()) {
        // Two launches per step in a streamed loop: the value network (its tiles add the lookahead reward and write the replay
        // state), then decision + transition + the humans' ORCA velocities of the NEXT decision (sarl_decide_step_kernel); the
        // first call after anything else touched the engine computes those velocities with a launch of its own.  Workgroup
        // geometries that kernel does not cover (several waves per workgroup, kd bookkeeping) and
        // CROWDNAV_AMD_SARL_FUSED_STEP=0: ORCA, the network with the decision by its last workgroup, the transition.
        const bool fused = s->fused_step;
        if (!C.const_vel && !(fused && fresh)) cn_launch_orca(e, s->orca_vel);
        // occupancy maps: the previous call's sarl_decide_step_kernel left next_obs / om behind its ORCA pass (fresh); otherwise
        // sarl_lookahead_kernel, a launch of its own like ORCA
        if (C.with_om && !(fused && fresh && !C.const_vel)) launch_lookahead(e);
        cn::SarlDecide D{};
        D.counter = fused ? nullptr : s->narrow_counter;
        D.epsilon = epsilon, D.alive = alive, D.done = done, D.best = best, D.action = action;
        D.state_out = state_out, D.env_stride = env_stride, D.sort_humans = sort_humans ? 1 : 0, D.in_dim = s->net.in_dim;
        D.reward = s->reward, D.value = s->narrow_value, D.gtime = e->S.gtime, D.mt_key = e->S.mt_key, D.mt_pos = e->S.mt_pos, D.error = e->C.error;
        if (C.with_om) D.next_obs_out = s->next_obs, D.om_out = s->om;
        // the replay-memory states on a workgroup of their own beside the tiles (CROWDNAV_AMD_SARL_SIDE_WG=0: on tile b's idle wave)
        static const bool side = env_int("CROWDNAV_AMD_SARL_SIDE_WG", 1) != 0;
        D.side_wg = (side && state_out) ? 1 : 0;
        launch_narrow(e, (unsigned)s->narrow_tiles + (unsigned)D.side_wg, D, s->V, C.with_om ? s->om : nullptr, nullptr);
        CN_HIP(hipGetLastError());
        if (fused) {
            const cn::StepIo io{action, reward, done, info, dmin, nullptr, nullptr, nullptr, 1};
            float* next_vel = C.const_vel ? nullptr : s->orca_vel;
            pick_maxl(e, [&](auto maxl) {
                pick_bool(e->P.robot_unicycle, [&](auto uni) {
                    hipLaunchKernelGGL((cn::sarl_decide_step_kernel<decltype(maxl)::value, decltype(uni)::value>), dim3(grid_envs(e)),
                                       dim3(e->P.threads), e->smem, e->stream, e->P, e->S, io, C, D, s->actions, next_vel);
                });
            });
            e->launch_counts[CN_COUNT_SARL_DECIDE_STEPS] += 1;
            CN_HIP(hipGetLastError());
            e->orca_fresh = next_vel != nullptr;
            return CN_OK;
        }
    } else {
        hipLaunchKernelGGL(cn::sarl_alive_kernel, dim3((C.B + 255) / 256), dim3(256), 0, e->stream, C.B, alive, done);
        if ((rc = cn_sarl_select(e, nullptr, best, action)) || (rc = cn_sarl_explore(e, epsilon, alive, best, action, nullptr)))
            return rc;
        if (state_out && (rc = cn_sarl_transform(e, state_out, env_stride, sort_humans))) return rc;
    }
    return cn_step(e, action, 1, reward, done, info, dmin, nullptr, nullptr, nullptr);
}

int cn_sarl_values(cn_engine* e, const float* states, int64_t n, float* out) {
    int rc = bind(e);
    if (rc) return rc;
    cn_sarl* s = e->sarl;
    if (!s || !s->weights_set) return fail(CN_ERR_INVALID, "cn_sarl_values: configure and set weights first");
    if (!states || !out) return fail(CN_ERR_INVALID, "cn_sarl_values: NULL argument");
    if (n < 1 || (uint64_t)n > (uint64_t)s->n_groups)
        return fail(CN_ERR_INVALID, "cn_sarl_values: %lld states, the engine's tiles hold 1 .. %zu (envs x actions)", (long long)n,
                    s->n_groups);
    if (!s->narrow() || s->net.in_dim != 13 || s->cfg.model == CN_MODEL_CADRL)
        return fail(CN_ERR_UNSUPPORTED, "cn_sarl_values: SARL / LSTM-RL on 13-wide rows at a size that takes the narrow tiles only");
    cn::SarlDecide D{};
    D.x_rows = states, D.ext_groups = (int)n, D.in_dim = s->net.in_dim;
    const int GT = cn::kSarlGroups / s->C.H;
    launch_narrow(e, (unsigned)((n + GT - 1) / GT), D, out, nullptr, nullptr);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_sarl_state_values(cn_engine* e, const double* state8, const double* theta, int64_t n, int sort_humans, float* value) {
    if (!state8) return fail(CN_ERR_INVALID, "cn_sarl_state_values: state8 is NULL");
    if (!value) return fail(CN_ERR_INVALID, "cn_sarl_state_values: value is NULL");
    if (n < 1) return fail(CN_ERR_INVALID, "cn_sarl_state_values: n must be >= 1 (got %lld)", (long long)n);
    if (!e) return fail(CN_ERR_INVALID, "cn_sarl_state_values: engine is NULL");
    int rc = state_values_check(e, "cn_sarl_state_values", theta != nullptr);
    if (rc || (rc = bind(e))) return rc;
    return state_values_run(e, state8, theta, n, sort_humans, value);
}

// cn_lookahead_values and cn_lookahead_paths_values: the extra checks, the lookahead (human_vel == NULL: cn_lookahead_actions,
// else cn_lookahead_paths), the values of the branch ends, the score
static int lookahead_values(cn_engine* e, const char* who, int n_steps, int n_candidates, const double* actions,
                            const double* human_vel, const cn_lookahead_out* out, int sort_humans, float* value, double* score) {
    int rc = cn_lookahead_check(e, n_steps, n_candidates, actions, out);  // cn_lookahead_actions' own checks and messages
    if (rc) return rc;
    if (!out->final_state8) return fail(CN_ERR_INVALID, "%s: out->final_state8 is NULL (the caller owns the branch states)", who);
    if (!value) return fail(CN_ERR_INVALID, "%s: value is NULL", who);
    if (!score) return fail(CN_ERR_INVALID, "%s: score is NULL", who);
    if ((rc = state_values_check(e, who, out->final_theta != nullptr))) return rc;
    if (n_steps == 0) return CN_OK;
    if ((rc = human_vel ? cn_lookahead_paths(e, n_steps, n_candidates, actions, human_vel, out)
                        : cn_lookahead_actions(e, n_steps, n_candidates, actions, out)))
        return rc;
    const int64_t branches = (int64_t)e->P.B * n_candidates;
    if ((rc = state_values_run(e, out->final_state8, out->final_theta, branches, sort_humans, value))) return rc;
    hipLaunchKernelGGL(cn::lookahead_score_kernel, dim3((unsigned)((branches + 255) / 256)), dim3(256), 0, e->stream, (size_t)branches,
                       (const double*)out->ret, (const uint8_t*)out->info, (const int32_t*)out->steps, (const float*)value,
                       (const double*)e->discount, e->discount_len, score);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_lookahead_values(cn_engine* e, int n_steps, int n_candidates, const double* actions, const cn_lookahead_out* out,
                        int sort_humans, float* value, double* score) {
    return lookahead_values(e, "cn_lookahead_values", n_steps, n_candidates, actions, nullptr, out, sort_humans, value, score);
}

int cn_lookahead_paths_values(cn_engine* e, int n_steps, int n_candidates, const double* actions, const double* human_vel,
                              const cn_lookahead_out* out, int sort_humans, float* value, double* score) {
    if (!human_vel) return fail(CN_ERR_INVALID, "cn_lookahead_paths_values: human_vel is NULL");
    return lookahead_values(e, "cn_lookahead_paths_values", n_steps, n_candidates, actions, human_vel, out, sort_humans, value, score);
}

int cn_sarl_export(cn_engine* e, int which, void* dst, uint64_t bytes) {
    int rc = bind(e);
    if (rc) return rc;
    cn_sarl* s = e->sarl;
    if (!s || !dst) return fail(CN_ERR_INVALID, "cn_sarl_export: not configured or NULL dst");
    const cn::SarlCfg& C = s->C;
    const void* src = nullptr;
    size_t have = 0;
    switch (which) {
        case 0: src = s->reward, have = sizeof(double) * s->n_groups; break;
        case 1: src = s->V, have = sizeof(float) * s->n_groups; break;
        case 2: src = s->next_obs, have = sizeof(double) * C.B * C.H * 5; break;
        case 3: src = s->om, have = sizeof(float) * C.B * C.H * (s->net.in_dim - 13); break;
        case 4:
            if (s->narrow()) {  // the network kernel built X in LDS: the same rows, for the caller who asks to see them
                launch_features(e, 1, s->orca_vel);
                CN_HIP(hipGetLastError());
            }
            if (s->pre) {  // the feature kernel wrote k-steps 0..3 only: the map columns from `om`
                const size_t rows = s->n_tiles * cn::kSarlGroups * C.H;
                hipLaunchKernelGGL(cn::sarl_om_columns_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream, C,
                                   s->net.in_dim, s->net.ks_x, s->om, s->X, s->n_tiles);
                CN_HIP(hipGetLastError());
            }
            src = s->X, have = sizeof(float) * s->n_tiles * C.H * s->net.ks_x * 64;
            break;
        default: return fail(CN_ERR_INVALID, "cn_sarl_export: unknown buffer %d", which);
    }
    if (bytes > have) return fail(CN_ERR_INVALID, "cn_sarl_export: buffer %d holds %zu bytes, %llu requested", which, have,
                                 (unsigned long long)bytes);
    CN_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, e->stream));
    return CN_OK;
}

}  // extern "C"

#ifdef CN_PHASE_TIMING
// profiling builds only (scripts/sarl_phase_probe.py)
extern "C" int cn_debug_sarl_cycles(unsigned long long* out16, int reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(cn::cn_sarl_cycles), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(cn::cn_sarl_cycles), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
