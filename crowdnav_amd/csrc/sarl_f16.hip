// The split-f16 route of the value network (CN_PRECISION_F16X2; sarl_f16_kernel.h): its weight stream, the packing and its
// launcher (sarl_host.h).
#include "sarl_host.h"
#include "sarl_f16_kernel.h"

int sarl_f16_alloc(cn_engine* e, cn_sarl* s) {
    const int xkb = cn::f16_key(s->net.in_dim == 13 ? 1 : 2, s->C.H);
    int rc;
    if ((rc = dev_alloc(e, &s->f16_stream, cn::f16_stream_bytes(xkb) / sizeof(_Float16))) ||
        (rc = dev_alloc(e, &s->f16_bias, (size_t)cn::f16_total_tiles(xkb) * 256)))
        return rc;
    return CN_OK;
}

// Wh / Wl in the matrix instruction's operand order, the biases in accumulator order: one launch
int sarl_f16_pack(cn_engine* e, const float* const* p) {
    const cn_sarl* s = e->sarl;
    cn::F16PackPlan plan{};
    plan.xkb = cn::f16_key(s->net.in_dim == 13 ? 1 : 2, s->C.H);
    for (int l = 0; l < 11; ++l) plan.W[l] = p[2 * l], plan.b[l] = p[2 * l + 1];
    const int total = cn::f16_total_items(plan.xkb) * 512 + cn::f16_total_tiles(plan.xkb) * 256;
    hipLaunchKernelGGL(cn::sarl_f16_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, e->stream, plan, s->f16_stream, s->f16_bias);
    CN_HIP(hipGetLastError());
    return CN_OK;
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
