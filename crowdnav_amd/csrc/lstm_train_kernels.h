// One SGD(momentum) step on lstm_rl.ValueNetwork1 (crowd_nav/policy/lstm_rl.py:9-33: an LSTM over the humans, hidden width 50,
// then the value head 56 -> 150 -> 100 -> 100 -> 1) in TWO launches, on the design of sarl_train_kernels.h.
//
//   lstm_train_tile_kernel  one workgroup per tile of 16 whole samples: rows of the tile are samples, the H humans are the
//                           LSTM's steps (the tiling sarl_narrow_kernel<true> uses for decisions).  Forward: the input half
//                           of every step's gates up front, the recurrence, the head through fwd_layer; backward: the head
//                           through bwd_layer, then back through time with dh_{t-1} = dGates_t W_hh on MFMA.  It leaves one
//                           dGates row [200] and one h_{t-1} row [50] per (sample, step), the head's input and
//                           pre-activation gradient rows per sample, and the tile's sum of squared errors in partial[tile].
//   train_update_kernel     as it is: six GradLayers (W_ih | b_ih over the ring's rows, W_hh | b_hh over the h_{t-1} rows,
//                           the head's four), the other five empty.
//
// Where the kept activations live.  Per step they are 16 x (200 gates + 50 c_t + 50 h_{t-1}) floats; at H = 8 the gates alone
// (16 x 200 x 8 = 100 KiB) do not fit beside the head's buffers.  So:
//   gates    in the SLAB, in the very rows the update kernel reads as dGates: the input half W_ih x_t + b_ih first, the
//            activated i f g o after the step, dGates after the step's backward — three uses, one row, and the last two by
//            the same thread.  200 x n x H floats (400 KiB at n = 100, H = 5): L2-resident.
//   h_{t-1}  in the slab as well (the update kernel needs the rows; the tile kernel itself only the current one, two LDS
//            buffers that swap).
//   c_t      in LDS for all steps (16 x 50 x 8 floats = 25 KiB): read twice in the backward, by every step.
//   tanh c_t not kept: recomputed from c_t, the same function of the same float.
// Torch's gate order i, f, g, o along the 200 rows of W_ih / W_hh.  No atomics; every value has one owner.
#pragma once
#include "sarl_train_kernels.h"

namespace cnt {

constexpr int kHid = 50, kGates = 4 * kHid;
constexpr int kLstmLayers = 6;   // W_ih, W_hh, mlp.0, mlp.2, mlp.4, mlp.6: (weight, bias) pairs P[2l], P[2l + 1]
constexpr int kLdC = 52;
static_assert(kSelf + kHid == kJoint, "the head's input is as wide as SARL's joint state");

// scratch rows the update kernel reads
struct LstmScratch {
    float* gates;                  // rows n*H [200]: input half -> i f g o -> dGates, in place
    float* hp;                     // rows n*H [50]: h_{t-1}, zero at the first step
    float *j, *q1, *q2, *q3;       // rows n: [56] [150] [100] [100]
    float *dD1, *dD2, *dD3, *dV;   // rows n: 150 100 100 1
};

// LDS map of one tile (floats)
constexpr int lX = 0;                                   // all steps' input rows, [step][sample], ld kLdX
constexpr int lPre = lX + kMaxH * kTileRows * kLdX;     // W_hh h_{t-1} + b_hh, later the step's dGates (A operand)
constexpr int lHa = lPre + kTileRows * kLd200;          // h_{t-1} / h_t, swapping
constexpr int lHb = lHa + kTileRows * kLd50;
constexpr int lC = lHb + kTileRows * kLd50;             // c_t of every step, ld kLdC
constexpr int lDC = lC + kMaxH * kTileRows * kLdC;      // dL/dc carried back through time
constexpr int lDH = lDC + kTileRows * kLdC;             // dL/dh_{t-1}
constexpr int lJ = lDH + kTileRows * kLd50;
constexpr int lQ1 = lJ + kTileRows * kLd50;
constexpr int lQ2 = lQ1 + kTileRows * kLd150;
constexpr int lQ3 = lQ2 + kTileRows * kLd100;
constexpr int lGA = lQ3 + kTileRows * kLd100;
constexpr int lGB = lGA + kTileRows * kLd200;
constexpr int lVL = lGB + kTileRows * kLd200;           // value / dV per sample, ld kLdS
constexpr int kLstmLdsFloats = lVL + kTileRows * kLdS;
static_assert(kLstmLdsFloats * 4 <= 160 * 1024, "tile does not fit the LDS of a gfx950 CU");

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// One half of the gates' pre-activations, sum_k A_t[r][k] W[o][k] + b[o], as steps x 13 independent 16 x 16 blocks dealt to
// the waves.  SLAB: the input half of all H steps (A_t = the step's input rows) straight to the slab's rows
// gates[(g0 + r) * H + t], valid rows only.  Otherwise one step's recurrent half into LDS, O[r][o], rows >= nvalid zero.
// (fwd_layer is not used here: a call with these widths changes how the compiler specialises it for train_tile_kernel.)
template <bool SLAB>
__device__ __forceinline__ void gate_half(const float* __restrict__ W, const float* __restrict__ b, int in, const float* A, int lda,
                                          int steps, float* O, int H, int g0, int nvalid, int wave, int nwaves, int lane) {
    const int c16 = lane & 15, kq = lane >> 4;
    constexpr int nblk = (kGates + 15) / 16;
    for (int job = wave; job < steps * nblk; job += nwaves) {
        const int t = job / nblk, nb = job - t * nblk;
        const int o = nb * 16 + c16;
        const bool ov = o < kGates;
        const float* wrow = W + (size_t)(ov ? o : 0) * in;
        const float* At = A + t * kTileRows * lda;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < in; k0 += 4 * kUnroll) {
            float av[kUnroll], bv[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int k = k0 + 4 * u + kq;
                const bool kv = k < in;
                av[u] = kv ? At[c16 * lda + k] : 0.f;
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
                const float v = acc[j] + bias;
                if (SLAB) {
                    if (row < nvalid) O[((size_t)(g0 + row) * H + t) * kGates + o] = v;
                } else {
                    O[row * kLd200 + o] = row < nvalid ? v : 0.f;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kTileThreads) void lstm_train_tile_kernel(const StepArgs a, const LstmScratch S) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kTileThreads / 64;
    const int H = a.H, D = a.D;
    const int s0 = blockIdx.x * kTileRows;            // first sample of the tile
    const int ns = min(kTileRows, a.n - s0);          // its samples = its valid rows
    float** P = const_cast<float**>(a.P);

    for (int i = tid; i < kLstmLdsFloats; i += kTileThreads) lds[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < ns * H * D; i += kTileThreads) {
        const int s = i / (H * D), rest = i - s * (H * D);
        const int t = rest / D, c = rest - t * D;
        lds[lX + (t * kTileRows + s) * kLdX + c] = a.states[ring_row(a, s0 + s) * H * D + rest];
    }
    __syncthreads();

    // ---- forward: the input half of all steps' gates, then the recurrence from h_0 = c_0 = 0
    gate_half<true>(P[0], P[1], D, lds + lX, kLdX, H, S.gates, H, s0, ns, wave, nw, lane);
    for (int t = 0; t < H; ++t) {
        float* hprev = lds + ((t & 1) ? lHb : lHa);
        float* hnext = lds + ((t & 1) ? lHa : lHb);
        gate_half<false>(P[2], P[3], kHid, hprev, kLd50, 1, lds + lPre, H, s0, ns, wave, nw, lane);
        __syncthreads();  // also orders the input half's slab rows before their readers
        for (int i = tid; i < ns * kHid; i += kTileThreads) {
            const int s = i / kHid, j = i - s * kHid;
            const size_t row = (size_t)(s0 + s) * H + t;
            float* g = S.gates + row * kGates;
            const float* pre = lds + lPre + s * kLd200;
            const float gi = sigmoidf(g[j] + pre[j]);
            const float gf = sigmoidf(g[kHid + j] + pre[kHid + j]);
            const float gg = tanhf(g[2 * kHid + j] + pre[2 * kHid + j]);
            const float go = sigmoidf(g[3 * kHid + j] + pre[3 * kHid + j]);
            const float cprev = t ? lds[lC + ((t - 1) * kTileRows + s) * kLdC + j] : 0.f;
            const float c = gf * cprev + gi * gg;
            g[j] = gi;
            g[kHid + j] = gf;
            g[2 * kHid + j] = gg;
            g[3 * kHid + j] = go;
            lds[lC + (t * kTileRows + s) * kLdC + j] = c;
            S.hp[row * kHid + j] = hprev[s * kLd50 + j];
            hnext[s * kLd50 + j] = go * tanhf(c);
        }
        __syncthreads();
    }
    const float* hlast = lds + ((H & 1) ? lHb : lHa);

    // ---- forward: the value head on [self state of row 0 | h_H]
    for (int i = tid; i < ns * kJoint; i += kTileThreads) {
        const int s = i / kJoint, c = i - s * kJoint;
        const float v = c < kSelf ? lds[lX + s * kLdX + c] : hlast[s * kLd50 + c - kSelf];
        lds[lJ + s * kLd50 + c] = v;
        S.j[(size_t)(s0 + s) * kJoint + c] = v;
    }
    __syncthreads();
    fwd_layer<true>(P[4], P[5], kM0, kJoint, lds + lJ, kLd50, lds + lQ1, kLd150, S.q1, kM0, s0, ns, wave, nw, lane);
    __syncthreads();
    fwd_layer<true>(P[6], P[7], kM1, kM0, lds + lQ1, kLd150, lds + lQ2, kLd100, S.q2, kM1, s0, ns, wave, nw, lane);
    __syncthreads();
    fwd_layer<true>(P[8], P[9], kM2, kM1, lds + lQ2, kLd100, lds + lQ3, kLd100, S.q3, kM2, s0, ns, wave, nw, lane);
    __syncthreads();
    fwd_layer<false>(P[10], P[11], 1, kM2, lds + lQ3, kLd100, lds + lVL, kLdS, nullptr, 0, 0, ns, wave, nw, lane);
    __syncthreads();

    // ---- loss and its gradient: mean over the n samples of (v - y)^2
    if (tid == 0) {
        double sq = 0.0;
        const float scale = 2.f / (float)a.n;
        for (int s = 0; s < ns; ++s) {
            const float diff = lds[lVL + s * kLdS] - a.values[ring_row(a, s0 + s)];
            sq += (double)diff * (double)diff;
            const float dv = scale * diff;
            lds[lVL + s * kLdS] = dv;
            S.dV[s0 + s] = dv;
        }
        a.S.partial[blockIdx.x] = sq;
    }
    __syncthreads();

    // ---- backward: the head; dJ ends in lGA, its columns 6.. are dL/dh_H
    bwd_layer(P[10], 1, kM2, lds + lVL, kLdS, lds + lGB, kLd200, lds + lQ3, kLd100, S.dD3, kM2, s0, ns, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[8], kM2, kM1, lds + lGB, kLd200, lds + lGA, kLd200, lds + lQ2, kLd100, S.dD2, kM1, s0, ns, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[6], kM1, kM0, lds + lGA, kLd200, lds + lGB, kLd200, lds + lQ1, kLd150, S.dD1, kM0, s0, ns, wave, nw, lane);
    __syncthreads();
    bwd_layer(P[4], kM0, kJoint, lds + lGB, kLd200, lds + lGA, kLd200, nullptr, 0, nullptr, 0, 0, ns, wave, nw, lane);
    __syncthreads();

    // ---- backward through time; lPre's rows >= ns are still the zeros the forward left there
    for (int t = H - 1; t >= 0; --t) {
        for (int i = tid; i < ns * kHid; i += kTileThreads) {
            const int s = i / kHid, j = i - s * kHid;
            float* g = S.gates + ((size_t)(s0 + s) * H + t) * kGates;
            float* dg = lds + lPre + s * kLd200;
            const float gi = g[j], gf = g[kHid + j], gg = g[2 * kHid + j], go = g[3 * kHid + j];
            const float tc = tanhf(lds[lC + (t * kTileRows + s) * kLdC + j]);
            const float cprev = t ? lds[lC + ((t - 1) * kTileRows + s) * kLdC + j] : 0.f;
            const float dh = t == H - 1 ? lds[lGA + s * kLd200 + kSelf + j] : lds[lDH + s * kLd50 + j];
            const float dc = lds[lDC + s * kLdC + j] + dh * go * (1.f - tc * tc);
            const float d_o = dh * tc * (go * (1.f - go));
            const float d_i = dc * gg * (gi * (1.f - gi));
            const float d_g = dc * gi * (1.f - gg * gg);
            const float d_f = dc * cprev * (gf * (1.f - gf));
            lds[lDC + s * kLdC + j] = dc * gf;
            g[j] = dg[j] = d_i;
            g[kHid + j] = dg[kHid + j] = d_f;
            g[2 * kHid + j] = dg[2 * kHid + j] = d_g;
            g[3 * kHid + j] = dg[3 * kHid + j] = d_o;
        }
        if (t == 0) break;
        __syncthreads();
        bwd_layer(P[2], kGates, kHid, lds + lPre, kLd200, lds + lDH, kLd50, nullptr, 0, nullptr, 0, 0, ns, wave, nw, lane);
        __syncthreads();
    }
}

}  // namespace cnt
