// Host-side memory check of the refusal paths of cn_lookahead_paths, cn_lookahead_paths_values, cn_plan_cem_paths and
// cn_plan_mppi_paths: a stand-alone program (its own main, no Python, no GPU needed) that calls them with NULL and dangling
// arguments.  Every call must be refused with the expected status and message WITHOUT reading through a pointer; built with
// the host sanitizers, a read through one of the dangling pointers below would be reported.
//
//   cd crowdnav_amd/csrc && mkdir -p ../../build/asan/units && for tu in $(basename -s .hip *.hip); do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize \
//           -Xarch_host -fsanitize=address,undefined -c $tu.hip -o ../../build/asan/units/$tu.o & done; wait     (every *.hip is a unit of the library)
//   clang++ -std=c++17 -g -I../../include -fsanitize=address,undefined -c ../../scripts/probes/lookahead_paths_refusals.cpp \
//         -o ../../build/asan/main.o          (hipcc's clang++: /opt/rocm/lib/llvm/bin/clang++)
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined ../../build/asan/units/*.o ../../build/asan/main.o \
//         -o ../../build/asan/lookahead_paths_refusals -ldl
//   ../../build/asan/lookahead_paths_refusals          # prints "ok: N refusals" and exits 0
//
// Host code only: never run under a GPU sanitizer, never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "crowdnav_amd.h"

static int failures = 0, made = 0;

static void expect(int rc, int want, const char* word, const char* what) {
    ++made;
    const char* msg = cn_last_error();
    if (rc != want || !msg || !std::strstr(msg, word)) {
        std::fprintf(stderr, "FAIL %s: status %d (want %d), message \"%s\" (want \"%s\")\n", what, rc, want, msg ? msg : "(null)", word);
        ++failures;
    }
}

int main() {
    // addresses nothing lives at: a refusal must not read through them
    double* const dangling = reinterpret_cast<double*>(static_cast<uintptr_t>(0x1000));
    float* const dangling_f = reinterpret_cast<float*>(static_cast<uintptr_t>(0x2000));
    cn_lookahead_out out{};
    out.ret = dangling, out.info = reinterpret_cast<uint8_t*>(dangling), out.steps = reinterpret_cast<int32_t*>(dangling);
    out.time = dangling, out.final_state8 = dangling, out.final_theta = dangling;
    cn_lookahead_out no_ret = out;
    no_ret.ret = nullptr;
    cn_lookahead_out no_time = out;
    no_time.time = nullptr;
    const cn_lookahead_out* const dangling_out = reinterpret_cast<const cn_lookahead_out*>(static_cast<uintptr_t>(0x3000));

    // cn_lookahead_paths: NULL human_vel before anything else — a dangling `out` beside it is not looked at
    expect(cn_lookahead_paths(nullptr, 4, 3, dangling, nullptr, dangling_out), CN_ERR_INVALID, "cn_lookahead_paths: human_vel is NULL", "paths/human_vel");
    expect(cn_lookahead_paths(nullptr, -1, 0, nullptr, nullptr, nullptr), CN_ERR_INVALID, "human_vel is NULL", "paths/everything NULL");
    expect(cn_lookahead_paths(nullptr, 4, 3, nullptr, dangling, dangling_out), CN_ERR_INVALID, "actions is NULL", "paths/actions");
    expect(cn_lookahead_paths(nullptr, 4, 3, dangling, dangling, nullptr), CN_ERR_INVALID, "out is NULL", "paths/out");
    expect(cn_lookahead_paths(nullptr, 4, 3, dangling, dangling, &no_ret), CN_ERR_INVALID, "out->ret is NULL", "paths/out->ret");
    expect(cn_lookahead_paths(nullptr, 4, 3, dangling, dangling, &no_time), CN_ERR_INVALID, "out->time is NULL", "paths/out->time");
    expect(cn_lookahead_paths(nullptr, -1, 3, dangling, dangling, &out), CN_ERR_INVALID, "n_steps must be >= 0", "paths/n_steps");
    expect(cn_lookahead_paths(nullptr, 4, 0, dangling, dangling, &out), CN_ERR_INVALID, "n_candidates must be >= 1", "paths/n_candidates");
    expect(cn_lookahead_paths(nullptr, 4, 3, dangling, dangling, &out), CN_ERR_INVALID, "engine is NULL", "paths/engine");
    expect(cn_lookahead_paths(nullptr, 0, 3, dangling, dangling, &out), CN_ERR_INVALID, "engine is NULL", "paths/engine, n = 0");

    // cn_lookahead_paths_values: the same, then nothing more without an engine
    expect(cn_lookahead_paths_values(nullptr, 4, 3, dangling, nullptr, dangling_out, 0, dangling_f, dangling), CN_ERR_INVALID,
           "cn_lookahead_paths_values: human_vel is NULL", "values/human_vel");
    expect(cn_lookahead_paths_values(nullptr, 4, 3, nullptr, dangling, dangling_out, 0, nullptr, nullptr), CN_ERR_INVALID, "actions is NULL",
           "values/actions");
    expect(cn_lookahead_paths_values(nullptr, 4, 3, dangling, dangling, &no_ret, 0, nullptr, nullptr), CN_ERR_INVALID, "out->ret is NULL",
           "values/out->ret");
    expect(cn_lookahead_paths_values(nullptr, 4, 3, dangling, dangling, &out, 0, nullptr, nullptr), CN_ERR_INVALID, "engine is NULL",
           "values/engine");

    // the planners: NULL human_vel first, then plan_check's refusals
    cn_plan_cfg cfg{};
    cfg.n_steps = 4, cfg.n_candidates = 5, cfg.n_elites = 2, cfg.iterations = 1, cfg.init_std = 0.3, cfg.seed = 1;
    cn_plan plan{};
    plan.mean = plan.std = plan.best_actions = plan.best_score = plan.action = plan.candidates = dangling;
    plan.look = out, plan.value = dangling_f, plan.score = dangling;
    cn_plan no_candidates = plan;
    no_candidates.candidates = nullptr;
    cn_plan_cfg boot = cfg;
    boot.bootstrap = 1;
    cn_plan no_value = plan;
    no_value.value = nullptr;
    const cn_plan_cfg* const dangling_cfg = reinterpret_cast<const cn_plan_cfg*>(static_cast<uintptr_t>(0x4000));
    const cn_plan* const dangling_plan = reinterpret_cast<const cn_plan*>(static_cast<uintptr_t>(0x5000));

    expect(cn_plan_cem_paths(nullptr, dangling_cfg, dangling_plan, nullptr, 0), CN_ERR_INVALID, "cn_plan_cem_paths: human_vel is NULL", "cem/human_vel");
    expect(cn_plan_cem_paths(nullptr, nullptr, dangling_plan, dangling, 0), CN_ERR_INVALID, "cn_plan_cem_paths: cfg is NULL", "cem/cfg");
    expect(cn_plan_cem_paths(nullptr, &cfg, nullptr, dangling, 0), CN_ERR_INVALID, "cn_plan_cem_paths: plan is NULL", "cem/plan");
    expect(cn_plan_cem_paths(nullptr, &cfg, &no_candidates, dangling, 0), CN_ERR_INVALID, "plan->candidates is NULL", "cem/candidates");
    expect(cn_plan_cem_paths(nullptr, &boot, &no_value, dangling, 0), CN_ERR_INVALID, "plan->value", "cem/value with bootstrap");
    expect(cn_plan_cem_paths(nullptr, &cfg, &plan, dangling, 0), CN_ERR_INVALID, "cn_plan_cem_paths: engine is NULL", "cem/engine");
    expect(cn_plan_cem_paths(nullptr, &boot, &plan, dangling, 0), CN_ERR_INVALID, "engine is NULL", "cem/engine with bootstrap");

    expect(cn_plan_mppi_paths(nullptr, dangling_cfg, dangling_plan, nullptr, 1.0, 0, 0), CN_ERR_INVALID, "cn_plan_mppi_paths: human_vel is NULL",
           "mppi/human_vel");
    expect(cn_plan_mppi_paths(nullptr, nullptr, &plan, dangling, 1.0, 0, 0), CN_ERR_INVALID, "cn_plan_mppi_paths: cfg is NULL", "mppi/cfg");
    expect(cn_plan_mppi_paths(nullptr, &cfg, &plan, dangling, 0.0, 0, 0), CN_ERR_INVALID, "temperature", "mppi/temperature");
    expect(cn_plan_mppi_paths(nullptr, &cfg, &plan, dangling, 1.0, 0, 0), CN_ERR_INVALID, "cn_plan_mppi_paths: engine is NULL", "mppi/engine");

    if (failures) {
        std::fprintf(stderr, "%d of %d refusals wrong\n", failures, made);
        return 1;
    }
    std::printf("ok: %d refusals\n", made);
    return 0;
}
