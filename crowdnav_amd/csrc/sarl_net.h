// The value network on FP32 MFMA (v_mfma_f32_16x16x4_f32: exact f32, k-ordered fma chain): what every kernel family that runs it
// shares: the constants, the packed layers, the configuration, the dense-layer building blocks and the profiling ticks.
// Templates and inline functions only, so that every value-network unit can include it; the kernels around the network
// (features, reward, selection) are sarl_kernels.h's.
//
// Row order inside an MLP tile is HUMAN-MAJOR: row = h * 16 + g (g = group within the tile).  A 16-row MFMA
// tile then holds human h of 16 different groups, so the per-group reductions of the network (mean over
// humans, masked softmax over humans, weighted feature sum) combine values at the same offset of different row
// tiles — no cross-lane traffic.
//
// Activations live in LDS in MFMA A-FRAGMENT ORDER: element (row tile rt, row r, feature n) of a buffer with
// `ks` k-steps per row tile sits at ((rt * ks + n / 4) * 64 + (n % 4) * 16 + r).  A wave then fetches the A operand
// of k-step s with lane l reading word (rt * ks + s) * 64 + l (conflict-free ds_read_b32), and the 4 accumulator
// values a lane owns (rows quad*4 .. quad*4+3 of one column) are 4 consecutive words: one ds_write_b128.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cn {

// CN_PHASE_TIMING (profiling builds only): per-layer shader-clock ticks of sarl_mlp_kernel as wave 0 sees them
// (barrier to barrier), summed over tiles into cn_sarl_cycles[k]; [15] = tiles.  scripts/sarl_phase_probe.py
#ifdef CN_PHASE_TIMING
static __device__ unsigned long long cn_sarl_cycles[16];
#define CN_SARL_CLOCK_BEGIN() unsigned long long sclk_last_ = __builtin_readcyclecounter(), sclk_acc_[15] = {}
#define CN_SARL_TICK(k)                                                  \
    do {                                                                 \
        const unsigned long long now_ = __builtin_readcyclecounter();    \
        sclk_acc_[k] += now_ - sclk_last_;                               \
        sclk_last_ = now_;                                               \
    } while (0)
#define CN_SARL_CLOCK_END_N(n_)                                                          \
    do {                                                                                 \
        if (threadIdx.x == 0) {                                                          \
            for (int k_ = 0; k_ < 15; ++k_) atomicAdd(&cn_sarl_cycles[k_], sclk_acc_[k_]); \
            atomicAdd(&cn_sarl_cycles[15], (unsigned long long)(n_));                    \
        }                                                                                \
    } while (0)
#define CN_SARL_CLOCK_END() CN_SARL_CLOCK_END_N(1)
#else
#define CN_SARL_CLOCK_BEGIN() \
    do {                      \
    } while (0)
#define CN_SARL_TICK(k) \
    do {                \
    } while (0)
#define CN_SARL_CLOCK_END() \
    do {                    \
    } while (0)
#define CN_SARL_CLOCK_END_N(n_) \
    do {                        \
    } while (0)
#endif

constexpr int kWaveSize = 64;        // gfx950 wavefront
constexpr int kSarlGroups = 16;      // (env, action) groups per MLP tile = MFMA tile height
constexpr int kSarlMaxHumans = 8;    // register arrays of the occupancy map / LSTM-RL ordering; more humans: SARL without maps
                                     // (sarl_mlp_chunked_kernel streams them; one-tile kernels hold up to 5 at the shipped widths)
constexpr int kSarlThreads = 1024;   // 16 waves per MLP workgroup (4 per SIMD: one wave's LDS/L2 waits hide behind the others' MFMAs)
constexpr int kSarlKChunk = 5;       // k-steps per trip of the MFMA loop (= B fragments prefetched at a time): K = 100 is 25 k-steps
constexpr int kSarlLayers = 12;      // packed linear layers (attention.0 is split into its two K halves)
constexpr int kSarlChunk = 5;        // row tiles per chunk of the streamed (any number of humans) kernels

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One packed linear layer: B-operand fragments of v_mfma_f32_16x16x4_f32, fragment (ct, ks) at
// w[(ct * kpad + ks) * 64 + lane] = W[n = ct*16 + (lane & 15)][k = ks*4 + (lane >> 4)] (0 outside), so a wave
// fetches a fragment with one coalesced 256-byte load; bias padded to ctiles * 16.
struct PackedLinear {
    const float* w;
    const float* bias;
    int K, N;       // true sizes
    int ksteps;     // ceil(K / 4)
    int kpad;       // ksteps rounded up to kSarlKChunk (zero fragments): the B prefetch never runs off the end
    int ctiles;     // ceil(N / 16)
};

// k-steps per row tile of an LDS activation buffer that holds n features: whole 16-column tiles of its producer, and
// at least the consumer's k loop (ksteps rounded up to kSarlKChunk) so that the straight-line loop stays inside the row
// tile.  The kernels zero their LDS once per tile: k-steps the producer never writes are finite (zero or stale
// activations) and meet zero weights.
__host__ __device__ inline int sarl_ks(int n) {
    const int tiles = (n + 15) / 16 * 4;
    const int kpad = ((n + 3) / 4 + kSarlKChunk - 1) / kSarlKChunk * kSarlKChunk;
    return tiles > kpad ? tiles : kpad;
}
// Word of feature k of row 0 of a row tile in fragment order; the caller adds the row.
__host__ __device__ __forceinline__ constexpr int tile_word(int k) { return (k >> 2) * 64 + (k & 3) * 16; }

enum {
    kL_mlp1_0, kL_mlp1_2, kL_mlp2_0, kL_mlp2_2, kL_att0_local, kL_att0_global, kL_att_2, kL_att_4,
    kL_mlp3_0, kL_mlp3_2, kL_mlp3_4, kL_mlp3_6
};

struct SarlNet {
    PackedLinear L[kSarlLayers];
    int in_dim;        // 13 or 13 + cell_num^2 * om_channel_size
    int with_global;   // sarl.py:17-21
    int H;
    // k-steps per row tile of the LDS buffers (fragment order): X input, wide hidden (A), mlp1 output (B),
    // per-human feature (C), scores (S)
    int ks_x, ks_a, ks_b, ks_c, ks_s;
};

// The same network as 12 x 3 dwords (offsets into ONE weight arena) for the persistent kernel, whose loop keeps every
// descriptor live in SGPRs: 12 PackedLinear structs (pointers, sizes) do not fit and spill through VGPRs into scratch.
struct LayerRef {
    uint32_t w, b;   // float offsets of the B fragments / the bias from SarlNetRef::base
    uint32_t dims;   // kpad | ctiles << 8 | ksteps << 16
};
struct SarlNetRef {
    const float* base;
    LayerRef L[kSarlLayers];
    int nf;            // mlp2 output width (per-human feature)
    int with_global;
    int ks_x, ks_a, ks_b, ks_c, ks_s;
};
__device__ __forceinline__ PackedLinear layer_of(const SarlNetRef& n, int l) {
    const LayerRef r = n.L[l];
    PackedLinear P;
    P.w = n.base + r.w, P.bias = n.base + r.b;
    P.K = 0, P.N = 0;
    P.kpad = (int)(r.dims & 0xffu), P.ctiles = (int)((r.dims >> 8) & 0xffu), P.ksteps = (int)(r.dims >> 16);
    return P;
}

struct SarlCfg {
    int B, H, n_actions;
    int with_om, cell_num, om_channels;
    int unicycle;  // actions are ActionRot(v, r): cadrl.py:119-125, crowd_sim.py:339-341
    int cadrl;           // cadrl.ValueNetwork (the row MLP + minimum over humans) instead of sarl.ValueNetwork: sarl_narrow_kernel's branch
    int const_vel;       // query_env = false (multi_human_rl.py:39-42): humans keep their velocity, reward = compute_reward
    int sort_lookahead;  // ... and the joint state LstmRL.predict sorted by decreasing distance feeds the network (lstm_rl.py:96-103)
    double cell_size;
    double dt, time_limit, success_reward, collision_penalty, discomfort_dist, discomfort_factor;
    double gamma_bar;  // pow(gamma, time_step * v_pref), computed on the host like multi_human_rl.py:52
};

// the jobs of sarl_pack_many_kernel (sarl_kernels.h): all layers of a network in one launch
constexpr int kPackJobs = 16;
struct PackJob {
    const float* W;
    const float* bias;
    float* wp;
    float* bp;
    int N, K, k_offset, k_count, kpad, ctiles, first_block;
};
struct PackJobs {
    PackJob job[kPackJobs];
    int n;
};

// ------------------------------------------------------------------------------------ value network
// Dense layer on MFMA: out[r][n] = act(bias[n] + extra[g][n] + sum_k in[r][k] W[n][k]) for r in [0, RT*16), buffers in
// fragment order (ks_in / ks_out k-steps per row tile).  A wave owns whole column tiles (ct = wave, wave + 16, ..)
// and all RT row tiles of them: per k-step it reads RT A fragments from LDS (conflict-free) and issues RT
// independent MFMAs; the B fragments of the next trip are already in flight from L2 (register double buffer).
// Workgroup barrier for data exchanged through LDS only: wait for this wave's LDS traffic, not for its global loads — so
// the B fragments of the NEXT layer, requested before the barrier (dense_prefetch), stay in flight across it
// (__syncthreads() drains vmcnt as well and would expose one L2 round trip per layer: 11 per tile).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Weights are read through GLOBAL-address-space pointers: a generic pointer whose provenance the compiler cannot see (the
// persistent kernel rebuilds them from an arena base) turns into flat_load, which counts on lgkmcnt as well as vmcnt — and
// lds_barrier's s_waitcnt lgkmcnt(0) would then wait for exactly the prefetch it is meant to leave in flight.
typedef const float __attribute__((address_space(1))) * gfloat_p;
__device__ __forceinline__ gfloat_p as_global(const float* p) { return (gfloat_p)p; }

// First trip of a wave's first column tile of a layer: kSarlKChunk B fragments + the bias, requested ahead of time.
struct BFrag {
    float b[kSarlKChunk];
    float bias;
};
__device__ __forceinline__ BFrag dense_prefetch(const PackedLinear& P, int wave, int lane) {
    BFrag f;
    const int ct = wave < P.ctiles ? wave : 0;  // waves without a column tile fetch tile 0 (no divergence, L2 hit)
    const gfloat_p wfrag = as_global(P.w) + (size_t)ct * P.kpad * 64 + lane;
#pragma unroll
    for (int j = 0; j < kSarlKChunk; ++j) f.b[j] = wfrag[j * 64];
    f.bias = as_global(P.bias)[ct * 16 + (lane & 15)];
    return f;
}

// wave0 / nwaves: the waves [wave0, wave0 + nwaves) share the layer's column tiles (default: the whole workgroup); the others
// return at once — the pipelined kernel runs two layers of different tiles side by side on disjoint wave ranges.
template <int RT, bool PRE = false>
__device__ __forceinline__ void dense_mfma(const PackedLinear& P, const float* in, int ks_in, float* out, int ks_out,
                                           bool relu, const float* extra, int wave, int lane, const BFrag* pre = nullptr,
                                           int wave0 = 0, int nwaves = kSarlThreads / 64) {
    const int col = lane & 15, quad = lane >> 4;
    if (wave < wave0 || wave >= wave0 + nwaves) return;
    for (int ct = wave - wave0; ct < P.ctiles; ct += nwaves) {
        // this lane's 4 accumulator rows of column n = ct*16 + col sit at 4 consecutive words of the out buffer
        const int frag_off = ((ct * 4 + (col >> 2)) * 64) + (col & 3) * 16 + quad * 4;
        // accumulators start at zero; bias (L2) and the per-group extra term (LDS) are requested now and added in the
        // epilogue, so their latency hides behind the k loop instead of opening the column tile
        f32x4 acc[RT];
        const bool first = PRE && ct == wave - wave0;  // this tile's first trip was prefetched before the barrier
        const float b0 = first ? pre->bias : as_global(P.bias)[ct * 16 + col];
        f32x4 addend = {b0, b0, b0, b0};
        if (extra) addend += *reinterpret_cast<const f32x4*>(extra + frag_off);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

        // Straight-line k loop, kSarlKChunk k-steps per trip, no conditionals (kpad <= ks_in by construction: every buffer
        // holds whole column tiles of its producer, zero beyond the true width, and the packed weights are zero
        // there too).  The B fragments of the next trip are requested before this trip's MFMAs issue; the
        // packed buffer carries one spare chunk so the last request stays in bounds.
        const gfloat_p wfrag = as_global(P.w) + (size_t)ct * P.kpad * 64 + lane;
        const float* afrag = in + lane;
        // One trip = kSarlKChunk k-steps x RT row tiles of MFMAs.  Its B fragments were requested from L2 a whole trip
        // earlier (bnxt; measured: a second trip of lead changes nothing).  Its A fragments come from LDS in two groups so
        // that no trip opens with a wait: the HEAD (first kHead k-steps) was requested during the previous trip, the REST
        // is requested now and arrives while the head's MFMAs run; then the next trip's head is requested while the
        // rest's MFMAs run.  (A whole second register set for A costs 25 VGPRs more and spills at 16 waves per CU.)
        // The head request after the last trip reads past the row tile into whatever follows it in LDS (always inside
        // the allocation: every MFMA input buffer is followed by another buffer) and is unused.
        constexpr int kHead = 2;
        float bcur[kSarlKChunk], bnxt[kSarlKChunk];
        float ah[kHead][RT], ar[kSarlKChunk - kHead][RT];
#pragma unroll
        for (int j = 0; j < kSarlKChunk; ++j) bcur[j] = first ? pre->b[j] : wfrag[j * 64];
#pragma unroll
        for (int j = 0; j < kHead; ++j)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) ah[j][rt] = afrag[(rt * ks_in + j) * 64];
        for (int k0 = 0; k0 < P.kpad; k0 += kSarlKChunk) {
#pragma unroll
            for (int j = 0; j < kSarlKChunk; ++j) bnxt[j] = wfrag[(k0 + kSarlKChunk + j) * 64];
#pragma unroll
            for (int j = kHead; j < kSarlKChunk; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) ar[j - kHead][rt] = afrag[(rt * ks_in + k0 + j) * 64];
            __builtin_amdgcn_sched_barrier(0);  // requests first
#pragma unroll
            for (int j = 0; j < kHead; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j][rt], bcur[j], acc[rt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < kHead; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) ah[j][rt] = afrag[(rt * ks_in + k0 + kSarlKChunk + j) * 64];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = kHead; j < kSarlKChunk; ++j)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[j - kHead][rt], bcur[j], acc[rt], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < kSarlKChunk; ++j) bcur[j] = bnxt[j];
            __builtin_amdgcn_sched_barrier(0);
        }
        // columns >= N of the last column tile are exact zeros (zero weights, zero bias): they are the consumer's
        // k padding, so they are stored too
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f32x4 v = acc[rt] + addend;
            if (relu) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.0f ? v[i] : 0.0f;
            }
            *reinterpret_cast<f32x4*>(out + rt * ks_out * 64 + frag_off) = v;
        }
    }
}

// ------------------------------------------------------------------------------------ steps shared between kernels
// What the narrow-tile and one-tile kernels must compute to the same bits (tests/test_sarl.py) is written once, here.
// A layer with ONE output (attention.4, mlp3.6) is a dot product on the vector ALUs: as an MFMA it would occupy one wave of one
// SIMD with 15 of 16 columns wasted (7 % of the tile time at 100 -> 1 over 5 row tiles).  A thread takes k-steps slice, slice +
// slices, .. of the row whose features start at in[row]; fragment (0, s): w[s * 64 + 16 j] = W[0][4 s + j].  (P by value in
// these three: through a reference hipcc allocates sarl_narrow_kernel's registers in another order.)
__device__ __forceinline__ float dot_k_slice(const PackedLinear P, const float* in, int row, int slice, int slices) {
    float sum = 0.0f;
    for (int s = slice; s < P.ksteps; s += slices) {
        const gfloat_p w = as_global(P.w) + s * 64;
        const float* x = in + s * 64 + row;
        sum += (x[0] * w[0] + x[16] * w[16]) + (x[32] * w[32] + x[48] * w[48]);
    }
    return sum;
}
// ... and the row's output: the bias, then its slices in order — from LDS (partial[s * stride + row]) or, four of them, by shuffles
__device__ __forceinline__ float fold_k_slices(const PackedLinear P, const float* partial, int stride, int row, int slices) {
    float v = as_global(P.bias)[0];
    for (int s = 0; s < slices; ++s) v += partial[s * stride + row];
    return v;
}
__device__ __forceinline__ float dot_on_one_wave(const PackedLinear P, const float* in, int lane) {
    const int row = lane & 15, slice = lane >> 4;  // 4 k slices of the 16 rows
    const float sum = dot_k_slice(P, in, row, slice, 4);
    float v = as_global(P.bias)[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) v += __shfl(sum, row + 16 * j);
    return v;
}
// Thread = (row, k slice) of RT row tiles; partial sums meet in `scratch` (kSarlThreads floats).  Contains one workgroup barrier.
template <int RT>
__device__ __forceinline__ void dense_vec1(const PackedLinear& P, const float* in, int ks_in, float* out, int ks_out,
                                           float* scratch, int tid) {
    constexpr int kRows = RT * 16, kSlices = kSarlThreads / kRows;
    const int row = tid % kRows, slice = tid / kRows;
    if (slice < kSlices) scratch[slice * kRows + row] = dot_k_slice(P, in + ((row >> 4) * ks_in) * 64 + (row & 15), 0, slice, kSlices);
    __syncthreads();
    if (tid < kRows) out[(tid >> 4) * ks_out * 64 + (tid & 15)] = fold_k_slices(P, scratch, kRows, tid, kSlices);
}
__device__ __forceinline__ void value_head_on_one_wave(const PackedLinear& P, const float* in, float* V, size_t tile,
                                                       int n_groups, int lane, int groups_per_tile = kSarlGroups) {
    const int row = lane & 15, slice = lane >> 4;  // dot_on_one_wave, spelled out: through the call sarl_mlp_pipe_kernel comes out with other registers
    const float sum = dot_k_slice(P, in, row, slice, 4);
    float v = as_global(P.bias)[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) v += __shfl(sum, row + 16 * j);
    const size_t G = tile * groups_per_tile + row;
    if (slice == 0 && row < groups_per_tile && G < (size_t)n_groups) V[G] = v;
}
// exp(score) of the softmax without max subtraction; a score of exactly zero is masked out (sarl.py:52-53)
__device__ __forceinline__ float masked_exp(float sc) { return expf(sc) * (sc != 0.0f ? 1.0f : 0.0f); }
// self_state = state[:, 0, :6] (sarl.py:36, lstm_rl.py:29): features 0..5 of the first `groups` rows of x -> the joint state
__device__ __forceinline__ void copy_self_state(float* jbuf, const float* x, int tid, int groups = kSarlGroups) {
    if (tid < kSarlGroups * 6 && (tid & 15) < groups) {
        const int g = tid & 15, n = tid >> 4;
        jbuf[tile_word(n) + g] = x[tile_word(n) + g];
    }
}
// torch.min over a group's humans (cadrl.py:162-163), the first minimum's value: m against v[h * stride + at] of the humans
// h in [from, n) that are present (h < cnt)
__device__ __forceinline__ float first_min_over_humans(const float* v, int stride, int at, int from, int n, int cnt, float m) {
    for (int h = from; h < n; ++h) {
        const float x = v[h * stride + at];
        m = (h < cnt && x < m) ? x : m;
    }
    return m;
}
__device__ __forceinline__ void zero_lds(float* lds, size_t words, int tid) {
    for (size_t i = tid; i < words; i += kSarlThreads) lds[i] = 0.0f;
}

}  // namespace cn
