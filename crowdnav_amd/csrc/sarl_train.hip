// cn_trainer_*: one SGD(momentum) step on sarl.ValueNetwork (sarl_train_kernels.h) or lstm_rl.ValueNetwork1
// (lstm_train_kernels.h) as two launches: the model's tile kernel, then the update kernel both share.  A trainer owns no
// environments and no copy of the parameters: only the scratch rows between its two kernels.  Third translation unit of
// libcrowdnav_amd.so; shares nothing with the other two but the error text.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/crowdnav_amd.h"
#include "lstm_train_kernels.h"
#include "sarl_train_kernels.h"

extern thread_local char cn_g_err[512];

namespace {

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(cn_g_err, sizeof(cn_g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define CNT_HIP(call)                                                                                          \
    do {                                                                                                       \
        hipError_t err__ = (call);                                                                             \
        if (err__ != hipSuccess)                                                                               \
            return fail(CN_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

}  // namespace

struct cn_trainer {
    int model, H, D, max_batch, device;
    hipStream_t stream = nullptr;
    bool ready = false;       // device probed, scratch allocated (first cn_train_step)
    float* slab = nullptr;    // every scratch row of cnt::Scratch
    cnt::Scratch S{};         // CN_MODEL_SARL's rows; `partial` serves both models
    cnt::LstmScratch LS{};    // CN_MODEL_LSTM_RL's rows
    int64_t steps = 0;
    int tensors() const { return 2 * (model == CN_MODEL_LSTM_RL ? cnt::kLstmLayers : cnt::kLayers); }
};

extern "C" {

int cn_trainer_create(const cn_sarl_config* net, int num_humans, int max_batch, int device, cn_trainer** out) {
    if (!net || !out) return fail(CN_ERR_INVALID, "cn_trainer_create: NULL net / out");
    *out = nullptr;
    if (net->model != CN_MODEL_SARL && net->model != CN_MODEL_LSTM_RL)
        return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: model %d: only CN_MODEL_SARL and CN_MODEL_LSTM_RL have a device SGD step",
                    net->model);
    static const int want1[2] = {cnt::kW1a, cnt::kW1b}, want2[2] = {cnt::kW2a, cnt::kW2b}, wanta[3] = {cnt::kAa, cnt::kAb, 1},
                     want3[4] = {cnt::kM0, cnt::kM1, cnt::kM2, 1}, wantl[2] = {cnt::kHid, 1}, none[4] = {0, 0, 0, 0};
    if (net->model == CN_MODEL_LSTM_RL) {  // compat/lstm_rl.py's convention: mlp1_dims = (hidden, 1), mlp3_dims = the head
        if (memcmp(net->interaction_dims, none, sizeof none))
            return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: interaction_dims (%d, %d, %d, %d): lstm_rl.ValueNetwork2 (the "
                        "interaction module) has no device SGD step", net->interaction_dims[0], net->interaction_dims[1],
                        net->interaction_dims[2], net->interaction_dims[3]);
        if (memcmp(net->mlp1_dims, wantl, sizeof wantl))
            return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: mlp1_dims (%d, %d): the device SGD step is built for an LSTM of "
                        "hidden width (50, 1)", net->mlp1_dims[0], net->mlp1_dims[1]);
    } else {
        if (!net->with_global_state)
            return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: with_global_state = 0 has no device SGD step");
        if (memcmp(net->mlp1_dims, want1, sizeof want1))
            return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: mlp1_dims (%d, %d): the device SGD step is built for (150, 100)",
                        net->mlp1_dims[0], net->mlp1_dims[1]);
        if (memcmp(net->mlp2_dims, want2, sizeof want2))
            return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: mlp2_dims (%d, %d): the device SGD step is built for (100, 50)",
                        net->mlp2_dims[0], net->mlp2_dims[1]);
        if (memcmp(net->attention_dims, wanta, sizeof wanta))
            return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: attention_dims (%d, %d, %d): the device SGD step is built for (100, 100, 1)",
                        net->attention_dims[0], net->attention_dims[1], net->attention_dims[2]);
    }
    if (memcmp(net->mlp3_dims, want3, sizeof want3))
        return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: mlp3_dims (%d, %d, %d, %d): the device SGD step is built for (150, 100, 100, 1)",
                    net->mlp3_dims[0], net->mlp3_dims[1], net->mlp3_dims[2], net->mlp3_dims[3]);
    if (net->with_om && (net->cell_num < 1 || net->om_channel_size < 1))
        return fail(CN_ERR_INVALID, "cn_trainer_create: with_om needs cell_num and om_channel_size >= 1");
    const long D = 13 + (net->with_om ? (long)net->cell_num * net->cell_num * net->om_channel_size : 0);
    if (D > cnt::kMaxD)
        return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: input width %ld (cell_num, om_channel_size) exceeds %d", D, cnt::kMaxD);
    if (num_humans < 1) return fail(CN_ERR_INVALID, "cn_trainer_create: num_humans %d < 1", num_humans);
    if (num_humans > cnt::kMaxH)
        return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: num_humans %d: the device SGD step takes up to %d", num_humans, cnt::kMaxH);
    if (max_batch < 1) return fail(CN_ERR_INVALID, "cn_trainer_create: max_batch %d < 1", max_batch);
    if (max_batch > cnt::kMaxBatch)
        return fail(CN_ERR_UNSUPPORTED, "cn_trainer_create: max_batch %d: the device SGD step takes up to %d", max_batch, cnt::kMaxBatch);
    if (device < 0) return fail(CN_ERR_INVALID, "cn_trainer_create: device %d out of range", device);
    cn_trainer* t = new (std::nothrow) cn_trainer();
    if (!t) return fail(CN_ERR_INVALID, "out of host memory");
    t->model = net->model;
    t->H = num_humans;
    t->D = (int)D;
    t->max_batch = max_batch;
    t->device = device;
    *out = t;
    return CN_OK;
}

int cn_trainer_destroy(cn_trainer* t) {
    if (!t) return CN_OK;
    if (t->slab) (void)hipFree(t->slab);
    delete t;
    return CN_OK;
}

int cn_trainer_set_stream(cn_trainer* t, void* hip_stream) {
    if (!t) return fail(CN_ERR_INVALID, "cn_trainer_set_stream: NULL trainer");
    t->stream = (hipStream_t)hip_stream;
    return CN_OK;
}

int cn_trainer_steps(const cn_trainer* t, int64_t* steps_host) {
    if (!t || !steps_host) return fail(CN_ERR_INVALID, "cn_trainer_steps: NULL trainer / steps_host");
    *steps_host = t->steps;
    return CN_OK;
}

}  // extern "C"

namespace {

struct LayerSpec { const float* dO; const float* A; int out, in, lda, rows; };

// first step: probe the device and carve the scratch rows out of one allocation
int trainer_prepare(cn_trainer* t) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(CN_ERR_NO_DEVICE, "no HIP device visible: the device SGD step has no CPU fallback");
    if (t->device >= ndev) return fail(CN_ERR_INVALID, "cn_train_step: device %d out of range", t->device);
    CNT_HIP(hipSetDevice(t->device));
    const bool lstm = t->model == CN_MODEL_LSTM_RL;
    if (lstm)
        CNT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cnt::lstm_train_tile_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, cnt::kLstmLdsFloats * (int)sizeof(float)));
    else
        CNT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cnt::train_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    cnt::kLdsFloats * (int)sizeof(float)));
    const size_t rh = (size_t)t->max_batch * t->H, rn = (size_t)t->max_batch;
    const size_t per_h = lstm ? cnt::kGates + cnt::kHid : 150 + 200 + 100 + 100 + 100 + 150 + 100 + 100 + 50 + 100 + 100 + 1;
    const size_t per_n = 56 + 150 + 100 + 100 + 150 + 100 + 100 + 1;
    const size_t floats = rh * per_h + rn * per_n + 2 * (size_t)cnt::kMaxBatch + 16;
    CNT_HIP(hipMalloc(&t->slab, floats * sizeof(float)));
    CNT_HIP(hipMemset(t->slab, 0, floats * sizeof(float)));
    float* p = t->slab;
    auto take = [&p](size_t n) { float* r = p; p += n; return r; };
    cnt::Scratch& S = t->S;
    S.partial = reinterpret_cast<double*>(take(2 * (size_t)cnt::kMaxBatch));  // first: 8-byte aligned
    if (lstm) {
        cnt::LstmScratch& L = t->LS;
        L.gates = take(rh * cnt::kGates); L.hp = take(rh * cnt::kHid);
        L.j = take(rn * 56); L.q1 = take(rn * 150); L.q2 = take(rn * 100); L.q3 = take(rn * 100);
        L.dD1 = take(rn * 150); L.dD2 = take(rn * 100); L.dD3 = take(rn * 100); L.dV = take(rn);
    } else {
        S.h1 = take(rh * 150); S.ai = take(rh * 200); S.g1 = take(rh * 100); S.k1 = take(rh * 100); S.k2 = take(rh * 100);
        S.dA1 = take(rh * 150); S.dA2 = take(rh * 100); S.dB1 = take(rh * 100); S.dF = take(rh * 50); S.dC1 = take(rh * 100);
        S.dC2 = take(rh * 100); S.dS = take(rh);
        S.j = take(rn * 56); S.q1 = take(rn * 150); S.q2 = take(rn * 100); S.q3 = take(rn * 100);
        S.dD1 = take(rn * 150); S.dD2 = take(rn * 100); S.dD3 = take(rn * 100); S.dV = take(rn);
    }
    t->ready = true;
    return CN_OK;
}

// the update kernel's layer list: `count` layers, the rest of its kLayers slots empty (no wave-block is theirs)
cnt::UpdateArgs update_args(const LayerSpec* spec, int count) {
    cnt::UpdateArgs u;
    int first = 0;
    for (int l = 0; l < cnt::kLayers; ++l) {
        cnt::GradLayer& L = u.L[l];
        const LayerSpec s = l < count ? spec[l] : LayerSpec{nullptr, nullptr, 0, 0, 0, 0};
        L.dO = s.dO; L.A = s.A; L.out = s.out; L.in = s.in; L.lda = s.lda; L.rows = s.rows;
        L.iblocks = (L.in + 1 + 15) / 16;
        L.first = first;
        first += (L.out + 15) / 16 * L.iblocks;
    }
    u.blocks = first;
    return u;
}

}  // namespace

extern "C" int cn_train_step(cn_trainer* t, float* const* params_host_array, float* const* momentum_host_array,
                             const float* states, const float* values, int64_t rows, const int64_t* index, int64_t n,
                             double lr, double momentum_factor, double* loss_sum) {
    if (!t) return fail(CN_ERR_INVALID, "cn_train_step: NULL trainer");
    if (!params_host_array || !momentum_host_array)
        return fail(CN_ERR_INVALID, "cn_train_step: NULL params_host_array / momentum_host_array");
    if (!states || !values) return fail(CN_ERR_INVALID, "cn_train_step: NULL states / values");
    if (n < 1) return fail(CN_ERR_INVALID, "cn_train_step: n %lld < 1", (long long)n);
    if (n > t->max_batch)
        return fail(CN_ERR_INVALID, "cn_train_step: n %lld exceeds max_batch %d", (long long)n, t->max_batch);
    if (rows < 1 || (!index && rows < n))
        return fail(CN_ERR_INVALID, "cn_train_step: rows %lld does not hold the batch", (long long)rows);
    const bool lstm = t->model == CN_MODEL_LSTM_RL;
    for (int k = 0; k < t->tensors(); ++k)
        if (!params_host_array[k] || !momentum_host_array[k])
            return fail(CN_ERR_INVALID, "cn_train_step: params_host_array / momentum_host_array entry %d is NULL", k);
    if (!t->ready) {
        const int rc = trainer_prepare(t);
        if (rc != CN_OK) return rc;
    }

    cnt::StepArgs a{};
    // state_dict order -> the (weight, bias) pairs the update kernel indexes as P[2l], P[2l + 1].  SARL's is that order;
    // lstm_rl.ValueNetwork1's is mlp.{0,2,4,6}.{weight,bias}, lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0.
    static const int lstm_order[2 * cnt::kLstmLayers] = {8, 10, 9, 11, 0, 1, 2, 3, 4, 5, 6, 7};
    for (int k = 0; k < t->tensors(); ++k) {
        const int from = lstm ? lstm_order[k] : k;
        a.P[k] = params_host_array[from];
        a.M[k] = momentum_host_array[from];
    }
    a.states = states;
    a.values = values;
    a.index = index;
    a.rows = rows;
    a.n = (int)n;
    a.H = t->H;
    a.D = t->D;
    a.samples_per_tile = lstm ? cnt::kTileRows : cnt::kTileRows / t->H;
    a.tiles = ((int)n + a.samples_per_tile - 1) / a.samples_per_tile;
    a.lr = (float)lr;
    a.mom = (float)momentum_factor;
    a.loss_sum = loss_sum;
    a.S = t->S;

    const int RH = (int)n * t->H, RN = (int)n;
    cnt::UpdateArgs u;
    if (lstm) {
        const cnt::LstmScratch& S = t->LS;
        const LayerSpec spec[cnt::kLstmLayers] = {
            {S.gates, nullptr, cnt::kGates, t->D, t->D, RH}, {S.gates, S.hp, cnt::kGates, cnt::kHid, cnt::kHid, RH},
            {S.dD1, S.j, 150, 56, 56, RN},                   {S.dD2, S.q1, 100, 150, 150, RN},
            {S.dD3, S.q2, 100, 100, 100, RN},                {S.dV, S.q3, 1, 100, 100, RN}};
        u = update_args(spec, cnt::kLstmLayers);
        hipLaunchKernelGGL(cnt::lstm_train_tile_kernel, dim3(a.tiles), dim3(cnt::kTileThreads), cnt::kLstmLdsFloats * sizeof(float),
                           t->stream, a, S);
    } else {
        const cnt::Scratch& S = t->S;
        const LayerSpec spec[cnt::kLayers] = {
            {S.dA1, nullptr, 150, t->D, t->D, RH}, {S.dA2, S.h1, 100, 150, 150, RH}, {S.dB1, S.ai, 100, 100, 200, RH},
            {S.dF, S.g1, 50, 100, 100, RH},        {S.dC1, S.ai, 100, 200, 200, RH}, {S.dC2, S.k1, 100, 100, 100, RH},
            {S.dS, S.k2, 1, 100, 100, RH},         {S.dD1, S.j, 150, 56, 56, RN},    {S.dD2, S.q1, 100, 150, 150, RN},
            {S.dD3, S.q2, 100, 100, 100, RN},      {S.dV, S.q3, 1, 100, 100, RN}};
        u = update_args(spec, cnt::kLayers);
        hipLaunchKernelGGL(cnt::train_tile_kernel, dim3(a.tiles), dim3(cnt::kTileThreads), cnt::kLdsFloats * sizeof(float), t->stream, a);
    }
    CNT_HIP(hipGetLastError());
    const int waves = cnt::kUpdateThreads / 64;
    hipLaunchKernelGGL(cnt::train_update_kernel, dim3((u.blocks + waves - 1) / waves), dim3(cnt::kUpdateThreads), 0, t->stream, a, u);
    CNT_HIP(hipGetLastError());
    ++t->steps;
    return CN_OK;
}
