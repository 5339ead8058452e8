// Host-side memory check of the refusal paths of cn_lookahead_modes, cn_plan_cem_modes and cn_plan_mppi_modes: a stand-alone
// program (its own main, no Python, no GPU needed) that calls them with NULL and dangling arguments.  Every call must be
// refused with the expected status and message WITHOUT reading through a device pointer; built with the host sanitizers, a read
// through one of the dangling pointers below would be reported.  (modes and out are HOST structs the call reads: they are real
// here, their pointer fields dangle.)
//
//   cd crowdnav_amd/csrc && mkdir -p ../../build/asan/units && for tu in $(basename -s .hip *.hip); do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize \
//           -Xarch_host -fsanitize=address,undefined -c $tu.hip -o ../../build/asan/units/$tu.o & done; wait     (every *.hip is a unit of the library)
//   clang++ -std=c++17 -g -I../../include -fsanitize=address,undefined -c ../../scripts/probes/lookahead_modes_refusals.cpp \
//         -o ../../build/asan/modes_main.o          (hipcc's clang++: /opt/rocm/lib/llvm/bin/clang++)
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined ../../build/asan/units/*.o ../../build/asan/modes_main.o \
//         -o ../../build/asan/lookahead_modes_refusals -ldl
//   ../../build/asan/lookahead_modes_refusals          # prints "ok: N refusals" and exits 0
//
// Host code only: never run under a GPU sanitizer, never loaded into Python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

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
    uint8_t* const dangling_b = reinterpret_cast<uint8_t*>(dangling);
    int32_t* const dangling_i = reinterpret_cast<int32_t*>(dangling);
    const cn_path_modes* const dangling_modes = reinterpret_cast<const cn_path_modes*>(static_cast<uintptr_t>(0x3000));
    const cn_modes_out* const dangling_out = reinterpret_cast<const cn_modes_out*>(static_cast<uintptr_t>(0x6000));

    cn_path_modes modes{};
    modes.n_modes = 3, modes.reduce = CN_MODES_MEAN, modes.risk_penalty = 0.5, modes.human_vel = dangling, modes.weight = dangling;
    cn_modes_out out{dangling, dangling, dangling_i, dangling_b, dangling_i, dangling, dangling, dangling_b, dangling_i, dangling};
    cn_modes_out bare{};
    bare.score = dangling;  // everything optional left out
    cn_modes_out no_score = out;
    no_score.score = nullptr;
    cn_path_modes m = modes;

    // 1. the pointers, in order; what stands beside the NULL one is not looked at
    expect(cn_lookahead_modes(nullptr, 4, 3, dangling, nullptr, dangling_out), CN_ERR_INVALID, "cn_lookahead_modes: modes is NULL", "modes");
    expect(cn_lookahead_modes(nullptr, -1, 0, nullptr, nullptr, nullptr), CN_ERR_INVALID, "modes is NULL", "everything NULL");
    m = modes, m.human_vel = nullptr, m.n_modes = 0;
    expect(cn_lookahead_modes(nullptr, 4, 3, dangling, &m, dangling_out), CN_ERR_INVALID, "modes->human_vel is NULL", "modes->human_vel");
    m = modes, m.n_modes = 0;
    expect(cn_lookahead_modes(nullptr, 4, 3, dangling, &m, nullptr), CN_ERR_INVALID, "cn_lookahead_modes: out is NULL", "out");
    expect(cn_lookahead_modes(nullptr, 4, 3, dangling, &m, &no_score), CN_ERR_INVALID, "out->score is NULL", "out->score");
    // 2. n_modes
    m = modes, m.n_modes = 0, m.reduce = 7;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_INVALID, "n_modes must be >= 1 (got 0)", "n_modes = 0");
    m.n_modes = -1;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_INVALID, "n_modes must be >= 1 (got -1)", "n_modes < 0");
    m.n_modes = 9;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_UNSUPPORTED, "n_modes = 9", "n_modes = 9");
    // 3. reduce
    m = modes, m.n_modes = 8, m.reduce = 2, m.risk_penalty = -1.0;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_INVALID, "reduce 2 unknown", "reduce = 2");
    m.reduce = -1;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_INVALID, "reduce -1 unknown", "reduce = -1");
    // 4. risk_penalty
    m = modes, m.reduce = CN_MODES_MIN, m.risk_penalty = -0.5;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_INVALID, "risk_penalty must be >= 0 and finite", "risk_penalty < 0");
    m.risk_penalty = INFINITY;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_INVALID, "risk_penalty must be >= 0 and finite", "risk_penalty inf");
    m.risk_penalty = NAN;
    expect(cn_lookahead_modes(nullptr, 4, 3, nullptr, &m, &out), CN_ERR_INVALID, "risk_penalty must be >= 0 and finite", "risk_penalty nan");
    // 5. cn_lookahead_actions' own, with its messages; with every optional array and with none
    for (const cn_modes_out* o : {static_cast<const cn_modes_out*>(&out), static_cast<const cn_modes_out*>(&bare)}) {
        m = modes;
        if (o == &bare) m.weight = nullptr, m.risk_penalty = 0.0;
        expect(cn_lookahead_modes(nullptr, -1, 0, nullptr, &m, o), CN_ERR_INVALID, "cn_lookahead_actions: actions is NULL", "actions");
        expect(cn_lookahead_modes(nullptr, -1, 0, dangling, &m, o), CN_ERR_INVALID, "n_steps must be >= 0 (got -1)", "n_steps");
        expect(cn_lookahead_modes(nullptr, 4, 0, dangling, &m, o), CN_ERR_INVALID, "n_candidates must be >= 1 (got 0)", "n_candidates");
        expect(cn_lookahead_modes(nullptr, 4, 3, dangling, &m, o), CN_ERR_INVALID, "cn_lookahead_actions: engine is NULL", "engine");
        expect(cn_lookahead_modes(nullptr, 0, 3, dangling, &m, o), CN_ERR_INVALID, "cn_lookahead_actions: engine is NULL", "engine, n = 0");
    }

    // the planners: NULL modes first, then plan_check's refusals; cn_lookahead_modes' own come behind the engine
    cn_lookahead_out look{};
    look.ret = dangling, look.info = dangling_b, look.steps = dangling_i, look.time = dangling, look.final_state8 = dangling, look.final_theta = dangling;
    cn_plan_cfg cfg{};
    cfg.n_steps = 4, cfg.n_candidates = 5, cfg.n_elites = 2, cfg.iterations = 1, cfg.init_std = 0.3, cfg.seed = 1;
    cn_plan plan{};
    plan.mean = plan.std = plan.best_actions = plan.best_score = plan.action = plan.candidates = dangling;
    plan.look = look, plan.value = dangling_f, plan.score = dangling;
    cn_plan no_candidates = plan;
    no_candidates.candidates = nullptr;
    cn_plan_cfg boot = cfg;
    boot.bootstrap = 1;
    cn_plan no_value = plan;
    no_value.value = nullptr;
    cn_path_modes bad = modes;
    bad.n_modes = 0;
    const cn_plan_cfg* const dangling_cfg = reinterpret_cast<const cn_plan_cfg*>(static_cast<uintptr_t>(0x4000));
    const cn_plan* const dangling_plan = reinterpret_cast<const cn_plan*>(static_cast<uintptr_t>(0x5000));

    expect(cn_plan_cem_modes(nullptr, dangling_cfg, dangling_plan, nullptr, 0), CN_ERR_INVALID, "cn_plan_cem_modes: modes is NULL", "cem/modes");
    expect(cn_plan_cem_modes(nullptr, nullptr, dangling_plan, dangling_modes, 0), CN_ERR_INVALID, "cn_plan_cem_modes: cfg is NULL", "cem/cfg");
    expect(cn_plan_cem_modes(nullptr, &cfg, nullptr, dangling_modes, 0), CN_ERR_INVALID, "cn_plan_cem_modes: plan is NULL", "cem/plan");
    expect(cn_plan_cem_modes(nullptr, &cfg, &no_candidates, dangling_modes, 0), CN_ERR_INVALID, "plan->candidates is NULL", "cem/candidates");
    expect(cn_plan_cem_modes(nullptr, &boot, &no_value, dangling_modes, 0), CN_ERR_INVALID, "plan->value", "cem/value with bootstrap");
    expect(cn_plan_cem_modes(nullptr, &cfg, &plan, dangling_modes, 0), CN_ERR_INVALID, "cn_plan_cem_modes: engine is NULL", "cem/engine");
    expect(cn_plan_cem_modes(nullptr, &cfg, &plan, &bad, 0), CN_ERR_INVALID, "cn_plan_cem_modes: engine is NULL", "cem/engine before n_modes");
    expect(cn_plan_cem_modes(nullptr, &boot, &plan, &modes, 0), CN_ERR_INVALID, "engine is NULL", "cem/engine with bootstrap");

    expect(cn_plan_mppi_modes(nullptr, dangling_cfg, dangling_plan, nullptr, 1.0, 0, 0), CN_ERR_INVALID, "cn_plan_mppi_modes: modes is NULL",
           "mppi/modes");
    expect(cn_plan_mppi_modes(nullptr, nullptr, &plan, dangling_modes, 1.0, 0, 0), CN_ERR_INVALID, "cn_plan_mppi_modes: cfg is NULL", "mppi/cfg");
    expect(cn_plan_mppi_modes(nullptr, &cfg, &plan, dangling_modes, 0.0, 0, 0), CN_ERR_INVALID, "temperature", "mppi/temperature");
    expect(cn_plan_mppi_modes(nullptr, &cfg, &plan, dangling_modes, 1.0, 0, 0), CN_ERR_INVALID, "cn_plan_mppi_modes: engine is NULL", "mppi/engine");

    if (failures) {
        std::fprintf(stderr, "%d of %d refusals wrong\n", failures, made);
        return 1;
    }
    std::printf("ok: %d refusals\n", made);
    return 0;
}
