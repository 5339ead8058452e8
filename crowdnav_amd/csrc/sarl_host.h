// Host interface of "the value network" between the units that run it: sarl_abi.hip (the cn_sarl_* entry points, the decision
// kernels, the narrow kernel, the route choice) and the units of the kernel families — sarl_reg.hip, sarl_reg_chunk.hip and
// sarl_reg_seq.hip (activations in registers), sarl_f16.hip (split-f16), sarl_lds.hip (activations in LDS).  A family's unit
// instantiates its kernels and is the only one that launches them; what it offers is below: size or allocate me at configure
// time, pack me at cn_sarl_set_weights time, launch me.  Plain C++ functions with hidden visibility: none of them is part of the
// library's ABI.
#pragma once
#include "engine_host.h"
#include "sarl_reg_stream.h"  // (sarl_net.h; kRegWaves, kRegHumans, kRegLstmHid for the grids and the route choice)

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
    size_t pipe_lds_bytes = 0;      // CN_MODEL_SARL: of sarl_mlp_pipe_kernel on the whole crowd, whether it fits or not
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

// What one launch of the network kernels evaluates: the first n_groups groups of X / hcount / V, on n_tiles tiles of kSarlGroups.
// A decision is the whole of the engine's buffers (whole_pass); cn_sarl_state_values fills them pass by pass, the last one shorter.
struct SarlPass {
    size_t n_groups, n_tiles;
};

namespace {

[[maybe_unused]] bool is_cadrl(const cn_sarl_config& c) { return c.model == CN_MODEL_CADRL; }
[[maybe_unused]] bool is_lstm(const cn_sarl_config& c) { return c.model == CN_MODEL_LSTM_RL; }
[[maybe_unused]] bool is_pairwise(const cn_sarl_config& c) { return is_lstm(c) && c.interaction_dims[0] > 0; }  // lstm_rl.ValueNetwork2

[[maybe_unused]] int bad_humans(int H) { return fail(CN_ERR_UNSUPPORTED, "value network on device: %d humans", H); }

// the persistent grid of a register-resident kernel: a wave per tile, at most per_cu workgroups (= waves per SIMD) per CU
[[maybe_unused]] dim3 reg_grid(const cn_sarl* s, const SarlPass& pass, unsigned per_cu) {
    const unsigned wgs = (unsigned)((pass.n_tiles + cn::kRegWaves - 1) / cn::kRegWaves), resident = (unsigned)s->n_cus * per_cu;
    return dim3(wgs < resident ? wgs : resident);
}
const dim3 kRegBlock(cn::kRegWaves * 64);

}  // namespace

#define CN_INTERNAL __attribute__((visibility("hidden")))

// sarl_lds.hip.  sarl_lds_size: the k-steps per row tile of the LDS buffers (net.ks_*), lds_bytes of the LDS kernel the
// configuration would run; *lds_chunked: that kernel is the chunked one, the humans do not fit one tile's LDS.
// launch_lds: LdsTile, LdsChunked — and the one-tile kernel of a configuration whose decisions take the narrow tiles.
CN_INTERNAL void sarl_lds_size(cn_sarl* s, bool* lds_chunked);
CN_INTERNAL int launch_lds(cn_engine* e, const SarlPass& pass, float* att);

// sarl_reg.hip: the five register-resident routes' weight streams (one packing kernel serves them all) and the launcher of
// RegSarl and RegSarlChunk (the hoisted occupancy-map term, then sarl_reg_kernel or launch_reg_chunk).  alloc: the route's streams
// and what else it keeps (s->route is set; e->sarl is not yet); pack: the state_dict `params` as those streams, beside the packed
// layers every configuration uploads.
CN_INTERNAL int sarl_reg_alloc(cn_engine* e, cn_sarl* s);
CN_INTERNAL int sarl_reg_pack(cn_engine* e, const float* const* params);
CN_INTERNAL int launch_reg(cn_engine* e, const SarlPass& pass, float* att);
// sarl_reg_chunk.hip: RegSarlChunk's kernel (launch_reg calls it)
CN_INTERNAL int launch_reg_chunk(cn_engine* e, const SarlPass& pass, float* att);
// sarl_reg_seq.hip: RegCadrl, RegLstm, RegLstm2 — the networks that take a group's humans one after another
CN_INTERNAL int launch_reg_seq(cn_engine* e, const SarlPass& pass);

// sarl_f16.hip (SplitF16)
CN_INTERNAL int sarl_f16_alloc(cn_engine* e, cn_sarl* s);
CN_INTERNAL int sarl_f16_pack(cn_engine* e, const float* const* params);
CN_INTERNAL int launch_split_f16(cn_engine* e, const SarlPass& pass, float* att);

// The network on the groups of `pass` as X / hcount hold them, V into s->V (sarl_abi.hip: the route's launcher)
CN_INTERNAL int launch_network(cn_engine* e, const SarlPass& pass, float* att);

#ifdef CN_PHASE_TIMING
// Profiling builds: cn::cn_sarl_cycles is a static device array, one copy per unit.  The units whose kernels tick (sarl_abi.hip:
// sarl_narrow_kernel; sarl_reg.hip: sarl_reg_kernel) each offer theirs — its ticks added to sum16 (unless NULL), the copy zeroed
// on `reset`, -1 if a copy fails — as one line over sarl_cycles_of; the other units' copies are never written or read.
CN_INTERNAL int sarl_abi_cycles(unsigned long long* sum16, int reset);
CN_INTERNAL int sarl_reg_cycles(unsigned long long* sum16, int reset);
// `symbol`: HIP_SYMBOL(cn::cn_sarl_cycles) as the calling unit sees it
template <class Symbol>
int sarl_cycles_of(const Symbol& symbol, unsigned long long* sum16, int reset) {
    unsigned long long mine[16] = {};
    if (sum16 && hipMemcpyFromSymbol(mine, symbol, sizeof(mine)) != hipSuccess) return -1;
    for (int k = 0; sum16 && k < 16; ++k) sum16[k] += mine[k];
    const unsigned long long zero[16] = {};
    return reset && hipMemcpyToSymbol(symbol, zero, sizeof(zero)) != hipSuccess ? -1 : 0;
}
#endif
