// One SGD(momentum) step on sarl.ValueNetwork (crowd_nav/policy/sarl.py:9-65, crowd_nav/utils/trainer.py:56-66) in TWO launches.
//
//   train_tile_kernel    one workgroup per tile of 16 / H whole samples (all H rows of a sample in one tile, so the mean-pool
//                        and the masked softmax stay inside it): forward with every post-activation kept in LDS, backward for
//                        the data gradients, both on v_mfma_f32_16x16x4_f32 with the weights read [out][in] as torch stores
//                        them.  It leaves each layer's input rows and pre-activation gradient rows in a scratch buffer and
//                        the tile's sum of squared errors (float64) in partial[tile].
//   train_update_kernel  one wave per 16 x 16 block of a layer's [out][in + 1] gradient (column `in` is the bias: its input
//                        is the constant 1): g = dOut^T A over ALL rows of the batch in row order, one MFMA accumulator chain,
//                        then buf = m * buf + g; p -= lr * buf on the caller's tensors.  Thread 0 adds the batch's MSE to
//                        loss_sum, partials in tile order.
//
// Nothing is summed across workgroups with atomics and no workgroup waits for another: every gradient entry has exactly one
// owner and one summation order, so a step is bitwise reproducible.  ReLU masks come from the kept post-activations
// (relu(a) > 0 <=> a > 0).  Shipped widths only (mlp1 150,100 / mlp2 100,50 / attention 100,100,1 / mlp3 150,100,100,1,
// with_global_state): they are compile-time constants here; the ABI refuses anything else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cnt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileRows = 16;
constexpr int kMaxD = 64;        // input width: 13 (+ occupancy maps), at most 64
constexpr int kMaxH = 8;
constexpr int kMaxBatch = 128;
constexpr int kLayers = 11;
constexpr int kTileThreads = 512;
constexpr int kUpdateThreads = 256;
constexpr int kUnroll = 4;       // k-steps whose operands are fetched before their MFMAs issue (a k-step past the end multiplies zeros)

// widths
constexpr int kW1a = 150, kW1b = 100, kW2a = 100, kW2b = 50, kAa = 100, kAb = 100, kM0 = 150, kM1 = 100, kM2 = 100;
constexpr int kSelf = 6, kJoint = kSelf + kW2b, kAttIn = 2 * kW1b;

// LDS row strides (floats), all = 4 mod 32 so that the 16 rows x 4 k of an A-operand read fall on distinct banks
constexpr int kLdX = 68, kLd150 = 164, kLd100 = 100, kLd200 = 228, kLd50 = 68, kLdS = 4;

// scratch rows the update kernel reads: per (sample, human) row and per sample
struct Scratch {
    float *h1, *ai, *g1, *k1, *k2;             // layer inputs, rows n*H: [150] [200 = h2 | mean h2] [100] [100] [100]
    float *dA1, *dA2, *dB1, *dF, *dC1, *dC2, *dS;  // pre-activation gradients, rows n*H: 150 100 100 50 100 100 1
    float *j, *q1, *q2, *q3;                   // rows n: [56] [150] [100] [100]
    float *dD1, *dD2, *dD3, *dV;               // rows n: 150 100 100 1
    double* partial;                           // [tiles] sum of (v - y)^2
};

struct StepArgs {
    float* P[2 * kLayers];   // weight, bias per layer in state_dict order
    float* M[2 * kLayers];   // their momentum buffers
    const float* states;     // [rows][H][D]
    const float* values;     // [rows]
    const int64_t* index;    // [n] or NULL
    int64_t rows;            // ring rows (indices are clamped into it: a bad index must not read outside the ring)
    int n, H, D, samples_per_tile, tiles;
    float lr, mom;
    double* loss_sum;
    Scratch S;
};

__device__ __forceinline__ int64_t ring_row(const StepArgs& a, int sample) {
    int64_t r = a.index ? a.index[sample] : (int64_t)sample;
    return r < 0 ? 0 : (r >= a.rows ? a.rows - 1 : r);
}

// O[r][o] = act(sum_k A[r][k] W[o][k] + b[o]) for the 16 rows of the tile; rows >= nvalid come out 0.  O in LDS, G (optional)
// the same rows in global scratch starting at row g0.
template <bool RELU>
__device__ __forceinline__ void fwd_layer(const float* __restrict__ W, const float* __restrict__ b, int out, int in,
                                          const float* A, int lda, float* O, int ldo, float* G, int ldg, int g0, int nvalid,
                                          int wave, int nwaves, int lane) {
    const int c16 = lane & 15, kq = lane >> 4;
    for (int nb = wave; nb * 16 < out; nb += nwaves) {
        const int o = nb * 16 + c16;
        const bool ov = o < out;
        const float* wrow = W + (size_t)(ov ? o : 0) * in;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < in; k0 += 4 * kUnroll) {  // operands of kUnroll k-steps first: their loads overlap
            float av[kUnroll], bv[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int k = k0 + 4 * u + kq;
                const bool kv = k < in;
                av[u] = kv ? A[c16 * lda + k] : 0.f;
                bv[u] = (kv && ov) ? wrow[k] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
        }
        if (ov) {
            const float bias = b[o];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 4 * kq + j;
                float v = acc[j] + bias;
                if (RELU) v = v > 0.f ? v : 0.f;
                if (row >= nvalid) v = 0.f;
                O[row * ldo + o] = v;
                if (G && row < nvalid) G[(size_t)(g0 + row) * ldg + o] = v;
            }
        }
    }
}

// dI[r][i] = (sum_o dO[r][o] W[o][i]) * [mask[r][i] > 0]; rows >= nvalid come out 0.
__device__ __forceinline__ void bwd_layer(const float* __restrict__ W, int out, int in, const float* dO, int ldd, float* dI,
                                          int ldi, const float* mask, int ldm, float* G, int ldg, int g0, int nvalid, int wave,
                                          int nwaves, int lane) {
    const int c16 = lane & 15, kq = lane >> 4;
    for (int nb = wave; nb * 16 < in; nb += nwaves) {
        const int i = nb * 16 + c16;
        const bool iv = i < in;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < out; k0 += 4 * kUnroll) {
            float av[kUnroll], bv[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int k = k0 + 4 * u + kq;
                const bool kv = k < out;
                av[u] = kv ? dO[c16 * ldd + k] : 0.f;
                bv[u] = (kv && iv) ? W[(size_t)k * in + i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
        }
        if (iv) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 4 * kq + j;
                float v = acc[j];
                if (mask && !(mask[row * ldm + i] > 0.f)) v = 0.f;
                if (row >= nvalid) v = 0.f;
                dI[row * ldi + i] = v;
                if (G && row < nvalid) G[(size_t)(g0 + row) * ldg + i] = v;
            }
        }
    }
}

// LDS map of one tile (floats)
constexpr int oX = 0;
constexpr int oH1 = oX + kTileRows * kLdX;
constexpr int oAI = oH1 + kTileRows * kLd150;
constexpr int oG1 = oAI + kTileRows * kLd200;
constexpr int oFE = oG1 + kTileRows * kLd100;
constexpr int oK1 = oFE + kTileRows * kLd50;
constexpr int oK2 = oK1 + kTileRows * kLd100;
constexpr int oJ = oK2 + kTileRows * kLd100;
constexpr int oQ1 = oJ + kTileRows * kLd50;
constexpr int oQ2 = oQ1 + kTileRows * kLd150;
constexpr int oQ3 = oQ2 + kTileRows * kLd100;
constexpr int oGA = oQ3 + kTileRows * kLd100;
constexpr int oGB = oGA + kTileRows * kLd200;
constexpr int oDH = oGB + kTileRows * kLd200;
constexpr int oDF = oDH + kTileRows * kLd100;
constexpr int oSC = oDF + kTileRows * kLd50;   // scores, then value / dV, ld kLdS
constexpr int oE = oSC + kTileRows * kLdS;     // exp(s) [s != 0]
constexpr int oWt = oE + kTileRows;            // softmax weight
constexpr int oZ = oWt + kTileRows;            // per sample: sum of e
constexpr int oDW = oZ + kTileRows;            // dL/dw per row
constexpr int oDS = oDW + kTileRows;           // dL/ds per row, ld kLdS
constexpr int oVL = oDS + kTileRows * kLdS;    // value / dV per sample, ld kLdS
constexpr int kLdsFloats = oVL + kTileRows * kLdS;
static_assert(kLdsFloats * 4 <= 160 * 1024, "tile does not fit the LDS of a gfx950 CU");

__global__ __launch_bounds__(kTileThreads) void train_tile_kernel(const StepArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kTileThreads / 64;
    const int H = a.H, D = a.D;
    const int s0 = blockIdx.x * a.samples_per_tile;                       // first sample of the tile
    const int ns = min(a.samples_per_tile, a.n - s0);                     // its samples
    const int nr = ns * H;                                                // its (sample, human) rows
    const int r0 = s0 * H;                                                // their first row in the scratch
    float** P = const_cast<float**>(a.P);

    for (int i = tid; i < kLdsFloats; i += kTileThreads) lds[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < nr * D; i += kTileThreads) {
        const int r = i / D, c = i - r * D;
        const int s = r / H, h = r - s * H;
        lds[oX + r * kLdX + c] = a.states[(ring_row(a, s0 + s) * H + h) * D + c];
    }
    __syncthreads();

    // ---- forward
    fwd_layer<true>(P[0], P[1], kW1a, D, lds + oX, kLdX, lds + oH1, kLd150, a.S.h1, kW1a, r0, nr, wave, nw, lane);
    __syncthreads();
    fwd_layer<true>(P[2], P[3], kW1b, kW1a, lds + oH1, kLd150, lds + oAI, kLd200, a.S.ai, kAttIn, r0, nr, wave, nw, lane);
    __syncthreads();
    for (int i = tid; i < ns * kW1b; i += kTileThreads) {  // global state: mean of mlp1's output over the humans of a sample
        const int s = i / kW1b, c = i - s * kW1b;
        float sum = 0.f;
        for (int h = 0; h < H; ++h) sum += lds[oAI + (s * H + h) * kLd200 + c];
        const float g = sum / (float)H;
        for (int h = 0; h < H; ++h) {
            lds[oAI + (s * H + h) * kLd200 + kW1b + c] = g;
            a.S.ai[(size_t)(r0 + s * H + h) * kAttIn + kW1b + c] = g;
        }
    }
    fwd_layer<true>(P[4], P[5], kW2a, kW1b, lds + oAI, kLd200, lds + oG1, kLd100, a.S.g1, kW2a, r0, nr, wave, nw, lane);
    __syncthreads();
    fwd_layer<false>(P[6], P[7], kW2b, kW2a, lds + oG1, kLd100, lds + oFE, kLd50, nullptr, 0, 0, nr, wave, nw, lane);
    fwd_layer<true>(P[8], P[9], kAa, kAttIn, lds + oAI, kLd200, lds + oK1, kLd100, a.S.k1, kAa, r0, nr, wave, nw, lane);
    __syncthreads();
    fwd_layer<true>(P[10], P[11], kAb, kAa, lds + oK1, kLd100, lds + oK2, kLd100, a.S.k2, kAb, r0, nr, wave, nw, lane);
    __syncthreads();
    fwd_layer<false>(P[12], P[13], 1, kAb, lds + oK2, kLd100, lds + oSC, kLdS, nullptr, 0, 0, nr, wave, nw, lane);
    __syncthreads();
    if (tid < ns) {  // the reference's masked softmax: e = exp(s) [s != 0], w = e / sum e  (sarl.py:52-53)
        float z = 0.f;
        for (int h = 0; h < H; ++h) {
            const float sc = lds[oSC + (tid * H + h) * kLdS];
            const float e = sc != 0.f ? expf(sc) : 0.f;
            lds[oE + tid * H + h] = e;
            z += e;
        }
        lds[oZ + tid] = z;
        for (int h = 0; h < H; ++h) lds[oWt + tid * H + h] = lds[oE + tid * H + h] / z;
    }
    __syncthreads();
    for (int i = tid; i < ns * kJoint; i += kTileThreads) {  // joint = [self state of row 0, weighted feature]
        const int s = i / kJoint, c = i - s * kJoint;
        float v;
        if (c < kSelf) {
            v = lds[oX + (s * H) * kLdX + c];
        } else {
            v = 0.f;
            for (int h = 0; h < H; ++h) v += lds[oWt + s * H + h] * lds[oFE + (s * H + h) * kLd50 + c - kSelf];
        }
        lds[oJ + s * kLd50 + c] = v;
        a.S.j[(size_t)(s0 + s) * kJoint + c] = v;
    }
    __syncthreads();
    fwd_layer<true>(P[14], P[15], kM0, kJoint, lds + oJ, kLd50, lds + oQ1, kLd150, a.S.q1, kM0, s0, ns, wave, nw, lane);
    __syncthreads();
    fwd_layer<true>(P[16], P[17], kM1, kM0, lds + oQ1, kLd150, lds + oQ2, kLd100, a.S.q2, kM1, s0, ns, wave, nw, lane);
    __syncthreads();
    fwd_layer<true>(P[18], P[19], kM2, kM1, lds + oQ2, kLd100, lds + oQ3, kLd100, a.S.q3, kM2, s0, ns, wave, nw, lane);
    __syncthreads();
    fwd_layer<false>(P[20], P[21], 1, kM2, lds + oQ3, kLd100, lds + oVL, kLdS, nullptr, 0, 0, ns, wave, nw, lane);
    __syncthreads();

    // ---- loss and its gradient: mean over the n samples of (v - y)^2
    if (tid == 0) {
        double sq = 0.0;
        const float scale = 2.f / (float)a.n;
        for (int s = 0; s < ns; ++s) {
            const float diff = lds[oVL + s * kLdS] - a.values[ring_row(a, s0 + s)];
            sq += (double)diff * (double)diff;
            const float dv = scale * diff;
            lds[oVL + s * kLdS] = dv;
            a.S.dV[s0 + s] = dv;
        }
        a.S.partial[blockIdx.x] = sq;
    }
    __syncthreads();

    // ---- backward
    bwd_layer(P[20], 1, kM2, lds + oVL, kLdS, lds + oGB, kLd200, lds + oQ3, kLd100, a.S.dD3, kM2, s0, ns, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[18], kM2, kM1, lds + oGB, kLd200, lds + oGA, kLd200, lds + oQ2, kLd100, a.S.dD2, kM1, s0, ns, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[16], kM1, kM0, lds + oGA, kLd200, lds + oGB, kLd200, lds + oQ1, kLd150, a.S.dD1, kM0, s0, ns, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[14], kM0, kJoint, lds + oGB, kLd200, lds + oGA, kLd200, nullptr, 0, nullptr, 0, 0, ns, wave, nw, lane);
    __syncthreads();
    for (int i = tid; i < nr * kW2b; i += kTileThreads) {  // weighted feature -> features
        const int r = i / kW2b, c = i - r * kW2b;
        const float v = lds[oWt + r] * lds[oGA + (r / H) * kLd200 + kSelf + c];
        lds[oDF + r * kLd50 + c] = v;
        a.S.dF[(size_t)(r0 + r) * kW2b + c] = v;
    }
    if (tid < nr) {  // ... -> weights
        float dw = 0.f;
        for (int c = 0; c < kW2b; ++c) dw += lds[oFE + tid * kLd50 + c] * lds[oGA + (tid / H) * kLd200 + kSelf + c];
        lds[oDW + tid] = dw;
    }
    __syncthreads();
    if (tid < ns) {  // masked softmax backward; the mask is a constant: ds = de e, de = dw / Z - sum_h(dw e) / Z^2
        const float z = lds[oZ + tid];
        float t = 0.f;
        for (int h = 0; h < H; ++h) t += lds[oDW + tid * H + h] * lds[oE + tid * H + h];
        const float back = t / (z * z);
        for (int h = 0; h < H; ++h) {
            const int r = tid * H + h;
            const float ds = (lds[oDW + r] / z - back) * lds[oE + r];
            lds[oDS + r * kLdS] = ds;
            a.S.dS[r0 + r] = ds;
        }
    }
    __syncthreads();
    bwd_layer(P[12], 1, kAb, lds + oDS, kLdS, lds + oGB, kLd200, lds + oK2, kLd100, a.S.dC2, kAb, r0, nr, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[10], kAb, kAa, lds + oGB, kLd200, lds + oGA, kLd200, lds + oK1, kLd100, a.S.dC1, kAa, r0, nr, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[8], kAa, kAttIn, lds + oGA, kLd200, lds + oGB, kLd200, nullptr, 0, nullptr, 0, 0, nr, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[6], kW2b, kW2a, lds + oDF, kLd50, lds + oGA, kLd200, lds + oG1, kLd100, a.S.dB1, kW2a, r0, nr, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[4], kW2a, kW1b, lds + oGA, kLd200, lds + oDH, kLd100, nullptr, 0, nullptr, 0, 0, nr, wave, nw, lane);
    __syncthreads();
    for (int i = tid; i < kTileRows * kW1b; i += kTileThreads) {  // mlp1's output: attention (direct + mean-pool / H) + mlp2
        const int r = i / kW1b, c = i - r * kW1b;
        float v = 0.f;
        if (r < nr) {
            const int s = r / H;
            float pool = 0.f;
            for (int h = 0; h < H; ++h) pool += lds[oGB + (s * H + h) * kLd200 + kW1b + c];
            v = lds[oGB + r * kLd200 + c] + pool / (float)H + lds[oDH + r * kLd100 + c];
            if (!(lds[oAI + r * kLd200 + c] > 0.f)) v = 0.f;
            a.S.dA2[(size_t)(r0 + r) * kW1b + c] = v;
        }
        lds[oGA + r * kLd200 + c] = v;
    }
    __syncthreads();
    bwd_layer(P[2], kW1b, kW1a, lds + oGA, kLd200, lds + oGB, kLd200, lds + oH1, kLd150, a.S.dA1, kW1a, r0, nr, wave, nw, lane);
}

// One layer's weight-gradient product as the update kernel sees it.
struct GradLayer {
    const float* dO;   // [rows][out]
    const float* A;    // [rows][lda]; NULL: the replay ring's rows through the index (mlp1.0)
    int out, in, lda, rows;
    int iblocks;       // ceil((in + 1) / 16)
    int first;         // first wave-block of this layer
};
struct UpdateArgs {
    GradLayer L[kLayers];
    int blocks;        // wave-blocks in all
};

__global__ __launch_bounds__(kUpdateThreads) void train_update_kernel(const StepArgs a, const UpdateArgs u) {
    const int lane = threadIdx.x & 63;
    const int wb = blockIdx.x * (kUpdateThreads / 64) + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.loss_sum) {
        double sq = 0.0;
        for (int t = 0; t < a.tiles; ++t) sq += a.S.partial[t];
        *a.loss_sum += sq / (double)a.n;
    }
    if (wb >= u.blocks) return;  // whole waves leave together
    int l = 0;
    while (l + 1 < kLayers && wb >= u.L[l + 1].first) ++l;
    const GradLayer& L = u.L[l];
    const int ob = (wb - L.first) / L.iblocks, ib = (wb - L.first) - ob * L.iblocks;
    const int c16 = lane & 15, kq = lane >> 4;
    const int o = ob * 16 + c16;   // A operand: dOut[r][o]
    const int i = ib * 16 + c16;   // B operand: input[r][i], column `in` = 1 (bias)
    const bool ov = o < L.out, iv = i < L.in, ib1 = i == L.in;
    const int H = a.H, D = a.D;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r4 = 0; r4 < L.rows; r4 += 4 * kUnroll) {
        float av[kUnroll], bv[kUnroll];
#pragma unroll
        for (int q = 0; q < kUnroll; ++q) {
            const int r = r4 + 4 * q + kq;
            const bool rv = r < L.rows;
            av[q] = (rv && ov) ? L.dO[(size_t)r * L.out + o] : 0.f;
            bv[q] = 0.f;
            if (rv && iv) {
                if (L.A) {
                    bv[q] = L.A[(size_t)r * L.lda + i];
                } else {
                    const int s = r / H, h = r - s * H;
                    bv[q] = a.states[(ring_row(a, s) * H + h) * D + i];
                }
            } else if (rv && ib1) {
                bv[q] = 1.f;
            }
        }
#pragma unroll
        for (int q = 0; q < kUnroll; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], acc, 0, 0, 0);
    }
    if (!(iv || ib1)) return;
    float* p = iv ? a.P[2 * l] : a.P[2 * l + 1];
    float* m = iv ? a.M[2 * l] : a.M[2 * l + 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int orow = ob * 16 + 4 * kq + j;
        if (orow >= L.out) continue;
        const size_t at = iv ? (size_t)orow * L.in + i : (size_t)orow;
        const float buf = a.mom * m[at] + acc[j];   // torch: buf.mul_(momentum).add_(grad); p.add_(buf, alpha=-lr)
        m[at] = buf;
        p[at] = p[at] - a.lr * buf;
    }
}

}  // namespace cnt
