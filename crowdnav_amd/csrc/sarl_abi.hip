// C ABI of the SARL robot decision (declared in include/crowdnav_amd.h): the cn_sarl_* entry points, validation, the route
// choice, the packed layers every route uploads, and the decision-side kernels — features, select, explore, transform, the
// narrow value-network kernel and the fused sampling step.  The other value-network kernels are instantiated, packed for and
// launched by units of their own (sarl_lds.hip, sarl_reg.hip, sarl_reg_chunk.hip, sarl_reg_seq.hip, sarl_f16.hip) behind sarl_host.h.
#include "sarl_host.h"
#include "sarl_kernels.h"
#include "sarl_narrow_kernel.h"
#include "sarl_step_fused.h"

void cn_sarl_release(cn_engine* e) {
    delete e->sarl;  // device buffers are owned by the engine's slabs
    e->sarl = nullptr;
}

namespace {

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

// The packed layers of the model, each with its place in the arena; the LDS buffers (k-steps per row tile) and the bytes of the LDS
// kernel (sarl_lds_size), the tile counts.  *lds_chunked: that kernel is the chunked one, the humans do not fit one tile's LDS.
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
    sarl_lds_size(s, lds_chunked);
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

// what the routes with weight streams of their own need beside the common buffers
int sarl_alloc_route(cn_engine* e, cn_sarl* s) {
    return s->route == SarlRoute::SplitF16 ? sarl_f16_alloc(e, s) : sarl_reg_alloc(e, s);
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

constexpr int kHeadLayers[4] = {cn::kL_mlp3_0, cn::kL_mlp3_2, cn::kL_mlp3_4, cn::kL_mlp3_6};

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
    if (is_lstm(s->cfg)) {  // lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0
        cn::PackedLinear& Li = s->net.L[cn::kL_mlp1_0];
        cn::PackedLinear& Lh = s->net.L[cn::kL_mlp1_2];
        if ((rc = sarl_pack(e, Li, p[8], p[10], Li.N, Li.K, 0)) || (rc = sarl_pack(e, Lh, p[9], p[11], Lh.N, Lh.K, 0))) return rc;
    }
    return CN_OK;
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

SarlPass whole_pass(const cn_sarl* s) { return SarlPass{s->n_groups, s->n_tiles}; }
SarlPass pass_of(size_t groups) { return SarlPass{groups, (groups + cn::kSarlGroups - 1) / cn::kSarlGroups}; }

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

// The network on the groups of `pass` as X / hcount hold them, V into s->V: the route's kernel; on a narrow-route engine (whose
// decisions never put X in HBM) the configuration's LDS one-tile kernel, whose packed layers every configuration uploads.
int launch_network(cn_engine* e, const SarlPass& pass, float* att) {
    const cn_sarl* s = e->sarl;
    switch (s->route) {
        case SarlRoute::RegSarl:
        case SarlRoute::RegSarlChunk: return launch_reg(e, pass, att);
        case SarlRoute::SplitF16: return launch_split_f16(e, pass, att);
        case SarlRoute::RegCadrl:
        case SarlRoute::RegLstm:
        case SarlRoute::RegLstm2: return launch_reg_seq(e, pass);
        case SarlRoute::Narrow:
        case SarlRoute::LdsChunked:
        case SarlRoute::LdsTile: return launch_lds(e, pass, att);
    }
    return CN_OK;
}

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
                        s->pipe_lds_bytes - sizeof(float) * 64 * (size_t)s->net.ks_a, sizeof(float) * 64 * (size_t)s->net.ks_a);
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
    // ... and the same parameters as the weight streams of a route that has its own
    if ((rc = s->route == SarlRoute::SplitF16 ? sarl_f16_pack(e, params_host_array) : sarl_reg_pack(e, params_host_array))) return rc;
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
// profiling builds only (scripts/sarl_phase_probe.py): cn_sarl_cycles is one copy per unit that holds ticking kernels — this
// one's (sarl_narrow_kernel) and sarl_reg.hip's (sarl_reg_kernel); the sum of the copies, all of them reset
int sarl_abi_cycles(unsigned long long* sum16, int reset) { return sarl_cycles_of(HIP_SYMBOL(cn::cn_sarl_cycles), sum16, reset); }
extern "C" int cn_debug_sarl_cycles(unsigned long long* out16, int reset) {
    unsigned long long sum[16] = {};
    if (sarl_abi_cycles(out16 ? sum : nullptr, reset) || sarl_reg_cycles(out16 ? sum : nullptr, reset)) return -1;
    if (out16) memcpy(out16, sum, sizeof(sum));
    return 0;
}
#endif
