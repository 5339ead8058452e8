// libcrowdnav_amd.so — the device CEM and MPPI planners (cn_plan_*): host entry points over the kernels of plan_kernels.h.
//
// A planner is a CALLER of the engine: candidates are scored through cn_lookahead_actions / cn_lookahead_values (the *_paths
// calls: cn_lookahead_paths / cn_lookahead_paths_values; the *_modes calls: cn_lookahead_modes) and real steps
// made through cn_rollout_step, by their C entry points and therefore with their checks, their scenario-ring fill and their
// launch counters; this translation unit only adds what runs between them (draw, refit or MPPI update, shift, prior, and the
// shipped predictors' table: cn_predict, in front of every planning step of the cn_plan_*_predict_rollout calls), enqueued on the
// engine's stream.  Nothing here synchronises, allocates or counts.
// cn_predict_orca (predict_orca_kernel.h) is instantiated here as well: the step kernels' workgroup stepping the humans alone, the
// third predictor beside cn_predict's two, and the *_predict_orca_rollout calls that write it over one slot of cn_predict's table.
// cn_predict_orca_robot is the same launch with the robot in the humans' sight on a table of actions; the *_nominal_rollout calls
// give it the plan's clipped mean, candidate 0 of the planning step's first draw.
// cn_predict_orca_goals is cn_predict_orca's table for M hypotheses about the humans' goals in one launch (the workgroup over B M
// virtual envs), and cn_goal_hypotheses the streaming kernel that samples such goals from the state.
// A CN_UNICYCLE engine is served once cn_plan_set_unicycle has named its rotation bound: rows (v, r), the *_uni_kernel forms of
// the reset, draw, MPPI update and shift; the refit is component-wise and the same kernel.
#include "engine_host.h"
#include "plan_kernels.h"
#include "predict_orca_kernel.h"

namespace {

// The MPPI update's two arguments; a NULL Mppi* below means the CEM refit.
struct Mppi {
    double temperature;
    int fit_std;
};

// The engine plans over (v, r): a CN_UNICYCLE engine whose caller has made cn_plan_set_unicycle (which refuses every other engine).
// The one place that decides between the holonomic kernels and the *_uni_kernel forms.
inline bool plan_unicycle(const cn_engine* e) { return e->plan_max_rotation > 0.0; }

// Refusals 1-5 of the header, in its order; nothing is enqueued (cn_lookahead_values with n_steps == 0 checks and returns).
// The cn_plan_mppi_* calls add theirs between the cfg ranges and the engine.
int plan_check(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const char* who, const Mppi* mppi = nullptr) {
    if (!cfg) return fail(CN_ERR_INVALID, "%s: cfg is NULL", who);
    if (!plan) return fail(CN_ERR_INVALID, "%s: plan is NULL", who);
    const bool boot = cfg->bootstrap != 0;
    const struct {
        const void* p;
        const char* name;
        bool required;
    } arrays[] = {{plan->mean, "mean", true},
                  {plan->std, "std", true},
                  {plan->best_actions, "best_actions", true},
                  {plan->best_score, "best_score", true},
                  {plan->action, "action", true},
                  {plan->candidates, "candidates", true},
                  {plan->look.ret, "look.ret", true},
                  {plan->look.info, "look.info", true},
                  {plan->look.steps, "look.steps", true},
                  {plan->look.time, "look.time", true},
                  {plan->look.final_state8, "look.final_state8 (required with bootstrap)", boot},
                  {plan->value, "value (required with bootstrap)", boot},
                  {plan->score, "score (required with bootstrap)", boot}};
    for (const auto& a : arrays)
        if (a.required && !a.p) return fail(CN_ERR_INVALID, "%s: plan->%s is NULL", who, a.name);
    if (cfg->n_steps < 1) return fail(CN_ERR_INVALID, "%s: n_steps must be >= 1 (got %d)", who, cfg->n_steps);
    if (cfg->n_steps > cn::kMaxDiscount)
        return fail(CN_ERR_UNSUPPORTED, "%s: n_steps = %d exceeds the %d steps the discount table covers", who, cfg->n_steps,
                    cn::kMaxDiscount);
    if (cfg->n_candidates < 2) return fail(CN_ERR_INVALID, "%s: n_candidates must be >= 2 (got %d)", who, cfg->n_candidates);
    if (cfg->n_candidates > cn::kPlanMaxCandidates)
        return fail(CN_ERR_UNSUPPORTED, "%s: n_candidates = %d exceeds the %d scores the refit kernel ranks in LDS", who,
                    cfg->n_candidates, cn::kPlanMaxCandidates);
    if (cfg->n_elites < 1) return fail(CN_ERR_INVALID, "%s: n_elites must be >= 1 (got %d)", who, cfg->n_elites);
    if (cfg->n_elites > cn::kPlanMaxElites)
        return fail(CN_ERR_UNSUPPORTED, "%s: n_elites = %d exceeds the %d elites the refit kernel holds", who, cfg->n_elites,
                    cn::kPlanMaxElites);
    if (cfg->n_elites > cfg->n_candidates)
        return fail(CN_ERR_INVALID, "%s: n_elites = %d exceeds n_candidates = %d", who, cfg->n_elites, cfg->n_candidates);
    if (cfg->iterations < 1) return fail(CN_ERR_INVALID, "%s: iterations must be >= 1 (got %d)", who, cfg->iterations);
    if (!(cfg->init_std > 0.0) || !std::isfinite(cfg->init_std))
        return fail(CN_ERR_INVALID, "%s: init_std must be > 0 and finite (got %g)", who, cfg->init_std);
    if (!(cfg->min_std >= 0.0) || !std::isfinite(cfg->min_std))
        return fail(CN_ERR_INVALID, "%s: min_std must be >= 0 and finite (got %g)", who, cfg->min_std);
    if (!(cfg->smoothing >= 0.0 && cfg->smoothing < 1.0))
        return fail(CN_ERR_INVALID, "%s: smoothing must be in [0, 1) (got %g)", who, cfg->smoothing);
    if (mppi && (!(mppi->temperature > 0.0) || !std::isfinite(mppi->temperature)))
        return fail(CN_ERR_INVALID, "%s: temperature must be > 0 and finite (got %g)", who, mppi->temperature);
    if (!e) return fail(CN_ERR_INVALID, "%s: engine is NULL", who);
    if (e->P.robot_orca) return fail(CN_ERR_INVALID, "%s is for CN_ROBOT_EXTERNAL engines (an ORCA robot takes no actions)", who);
    // (the gate: pinned behaviour until the caller names the rotation bound — a choice of theirs, not a fact of the environment)
    if (e->P.robot_unicycle && !plan_unicycle(e))
        return fail(CN_ERR_UNSUPPORTED, "%s: CN_UNICYCLE engines are not served: the plan is a Gaussian over (vx, vy) clipped to "
                    "the speed disc; one over (v, r) needs its own clip rule.  cn_plan_set_unicycle names it (the rotation bound and "
                    "the rotation deviation) and opts this engine in", who);
    if (cfg->bootstrap)
        return cn_lookahead_values(e, 0, cfg->n_candidates, plan->candidates, &plan->look, cfg->sort_humans, plan->value, plan->score);
    return cn_lookahead_check(e, cfg->n_steps, cfg->n_candidates, plan->candidates, &plan->look);
}

// the *_modes planners, behind plan_check: no bootstrap form (the branch-end states are per mode), then cn_lookahead_modes' own
// refusals without enqueuing (zero steps: it checks and returns)
int plan_check_modes(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const cn_path_modes* modes, const char* who) {
    if (cfg->bootstrap)
        return fail(CN_ERR_UNSUPPORTED, "%s: bootstrap is not served: the branch-end states are per mode and not kept", who);
    const cn_modes_out out{plan->look.ret, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return cn_lookahead_modes(e, 0, cfg->n_candidates, plan->candidates, modes, &out);
}

// ... and refusal 6: what cn_rollout_step refuses for the io block, without enqueuing (cn_rollout_actions of zero steps runs
// the io checks of every rollout entry point and launches nothing; the renumbering rule is upload_io's)
int plan_check_io(cn_engine* e, const cn_rollout_io* io, const cn_plan* plan) {
    const int rc = cn_rollout_actions(e, io, 0, plan->action, nullptr);
    if (rc) return rc;
    if (e->rollout_begun && (io->seed_base != e->begin_seed_base || io->seed_mod != e->begin_seed_mod))
        return fail(CN_ERR_INVALID, "rollout io: seed_base / seed_mod (%u / %u) differ from cn_rollout_begin's (%u / %u); call "
                    "cn_rollout_begin to renumber the episodes", io->seed_base, io->seed_mod, e->begin_seed_base, e->begin_seed_mod);
    return CN_OK;
}

inline unsigned plan_grid(size_t lanes) { return (unsigned)((lanes + cn::kPlanBlock - 1) / cn::kPlanBlock); }

int run_reset(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const uint8_t* mask) {
    const cn::Params& P = e->P;
    if (plan_unicycle(e))  // lane = env: the prior is a recurrence in t
        hipLaunchKernelGGL(cn::plan_reset_uni_kernel, dim3(plan_grid((size_t)P.B)), dim3(cn::kPlanBlock), 0, e->stream, P.B, P.A,
                           cfg->n_steps, P.dt, cfg->init_std, e->plan_std_rotation, e->plan_max_rotation, (const double2*)e->S.pos,
                           (const double2*)e->S.goal, (const double2*)e->S.rv, (const double*)e->S.theta, mask, (double2*)plan->mean,
                           (double2*)plan->std);
    else
        hipLaunchKernelGGL(cn::plan_reset_kernel, dim3(plan_grid((size_t)P.B * cfg->n_steps)), dim3(cn::kPlanBlock), 0, e->stream, P.B,
                           P.A, cfg->n_steps, P.dt, cfg->init_std, (const double2*)e->S.pos, (const double2*)e->S.goal,
                           (const double2*)e->S.rv, mask, (double2*)plan->mean, (double2*)plan->std);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int run_draw(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter) {
    const cn::Params& P = e->P;
    const size_t rows = (size_t)P.B * cfg->n_candidates * cfg->n_steps;  // (below 2^59 and B K within an int: cn_lookahead_check)
    const uint32_t seed_lo = (uint32_t)(cfg->seed & 0xffffffffu), seed_hi = (uint32_t)(cfg->seed >> 32);
    if (plan_unicycle(e))
        hipLaunchKernelGGL(cn::plan_draw_uni_kernel, dim3(plan_grid(rows)), dim3(cn::kPlanBlock), 0, e->stream, P.B, P.A,
                           cfg->n_candidates, cfg->n_steps, seed_lo, seed_hi, counter, e->plan_max_rotation, (const double2*)e->S.rv,
                           (const double2*)plan->mean, (const double2*)plan->std, (double2*)plan->candidates);
    else
        hipLaunchKernelGGL(cn::plan_draw_kernel, dim3(plan_grid(rows)), dim3(cn::kPlanBlock), 0, e->stream, P.B, P.A, cfg->n_candidates,
                           cfg->n_steps, seed_lo, seed_hi, counter, (const double2*)e->S.rv, (const double2*)plan->mean,
                           (const double2*)plan->std, (double2*)plan->candidates);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int run_refit(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, int keep_best) {
    hipLaunchKernelGGL(cn::plan_refit_kernel, dim3(e->P.B), dim3(64), 0, e->stream, cfg->n_candidates, cfg->n_steps, cfg->n_elites,
                       keep_best ? 1 : 0, cfg->smoothing, cfg->min_std, (const double*)(cfg->bootstrap ? plan->score : plan->look.ret),
                       (const double2*)plan->candidates, plan->mean, plan->std, (double2*)plan->best_actions, plan->best_score,
                       (double2*)plan->action, plan->order);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int run_mppi_update(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const Mppi& mppi, int keep_best) {
    const double* score = cfg->bootstrap ? plan->score : plan->look.ret;
    if (plan_unicycle(e))
        hipLaunchKernelGGL(cn::plan_mppi_uni_kernel, dim3(e->P.B), dim3(64), 0, e->stream, e->P.A, cfg->n_candidates, cfg->n_steps,
                           mppi.fit_std ? 1 : 0, keep_best ? 1 : 0, mppi.temperature, cfg->smoothing, cfg->min_std,
                           e->plan_max_rotation, score, (const double2*)plan->candidates, (const double2*)e->S.rv, plan->mean,
                           plan->std, (double2*)plan->best_actions, plan->best_score, (double2*)plan->action, plan->order);
    else
        hipLaunchKernelGGL(cn::plan_mppi_kernel, dim3(e->P.B), dim3(64), 0, e->stream, e->P.A, cfg->n_candidates, cfg->n_steps,
                           mppi.fit_std ? 1 : 0, keep_best ? 1 : 0, mppi.temperature, cfg->smoothing, cfg->min_std, score,
                           (const double2*)plan->candidates, (const double2*)e->S.rv, plan->mean, plan->std,
                           (double2*)plan->best_actions, plan->best_score, (double2*)plan->action, plan->order);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// One planning step of either planner: draw, score, update, `iterations` times.  human_vel (optional): the candidates are
// scored by the paths lookahead against the caller's predicted human motion instead of the engine's human model.  modes
// (optional, never with human_vel or bootstrap): by cn_lookahead_modes against the caller's M futures — look.ret receives the
// reduced score, which the updates rank, and look.info / steps / time the worst mode's rows.
// drawn: the caller has made iteration 0's draw already (run_rollout's nominal form), with that counter.
int run_plan(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter, const Mppi* mppi,
             const double* human_vel = nullptr, const cn_path_modes* modes = nullptr, bool drawn = false) {
    const int n = cfg->n_steps, K = cfg->n_candidates;
    const cn_modes_out worst{plan->look.ret, nullptr, nullptr, plan->look.info, plan->look.steps, plan->look.time,
                             nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < cfg->iterations; ++i) {
        int rc = (drawn && i == 0) ? CN_OK : run_draw(e, cfg, plan, counter + (uint32_t)i);
        if (rc) return rc;
        if (modes)
            rc = cn_lookahead_modes(e, n, K, plan->candidates, modes, &worst);
        else if (human_vel)
            rc = cfg->bootstrap ? cn_lookahead_paths_values(e, n, K, plan->candidates, human_vel, &plan->look, cfg->sort_humans,
                                                            plan->value, plan->score)
                                : cn_lookahead_paths(e, n, K, plan->candidates, human_vel, &plan->look);
        else
            rc = cfg->bootstrap ? cn_lookahead_values(e, n, K, plan->candidates, &plan->look, cfg->sort_humans, plan->value, plan->score)
                                : cn_lookahead_actions(e, n, K, plan->candidates, &plan->look);
        if (rc || (rc = mppi ? run_mppi_update(e, cfg, plan, *mppi, i > 0) : run_refit(e, cfg, plan, i > 0))) return rc;
    }
    return CN_OK;
}

int run_shift(cn_engine* e, const cn_rollout_io* io, const cn_plan_cfg* cfg, const cn_plan* plan) {
    const cn::Params& P = e->P;
    if (plan_unicycle(e))
        hipLaunchKernelGGL(cn::plan_shift_uni_kernel, dim3(plan_grid((size_t)2 * P.B)), dim3(cn::kPlanBlock), 0, e->stream, P.B, P.A,
                           cfg->n_steps, P.dt, cfg->init_std, e->plan_std_rotation, e->plan_max_rotation, (const double2*)e->S.pos,
                           (const double2*)e->S.goal, (const double2*)e->S.rv, (const double*)e->S.theta, (const uint8_t*)io->active,
                           (const int32_t*)io->cur_steps, plan->mean, plan->std);
    else
        hipLaunchKernelGGL(cn::plan_shift_kernel, dim3(plan_grid((size_t)2 * P.B)), dim3(cn::kPlanBlock), 0, e->stream, P.B, P.A,
                           cfg->n_steps, P.dt, cfg->init_std, (const double2*)e->S.pos, (const double2*)e->S.goal,
                           (const double2*)e->S.rv, (const uint8_t*)io->active, (const int32_t*)io->cur_steps, plan->mean, plan->std);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// The device predictors of a call, checked: M and the CN_PREDICT_* values of its modes as predict_kernel's argument word
struct Predict {
    int n_modes = 0;
    uint32_t models = 0;
};

// n_modes and the models, in the header's order; nothing else of the call is looked at
int predict_check_models(int n_modes, const int32_t* model, const char* who, Predict* out) {
    if (n_modes < 1) return fail(CN_ERR_INVALID, "%s: n_modes must be >= 1 (got %d)", who, n_modes);
    if (n_modes > cn::kPredictMaxModes)
        return fail(CN_ERR_UNSUPPORTED, "%s: n_modes = %d exceeds the %d modes of a table", who, n_modes, cn::kPredictMaxModes);
    out->n_modes = n_modes, out->models = 0;
    for (int m = 0; m < n_modes; ++m) {
        if (model[m] != CN_PREDICT_CONSTANT_VELOCITY && model[m] != CN_PREDICT_TO_GOAL)
            return fail(CN_ERR_INVALID, "%s: model[%d] = %d unknown (CN_PREDICT_CONSTANT_VELOCITY = 0, CN_PREDICT_TO_GOAL = 1)", who, m,
                        model[m]);
        out->models |= cn::predict_model_bits(m, (uint32_t)model[m]);
    }
    return CN_OK;
}

// ... and the table's size: predict_kernel indexes rows with size_t, the grid counts workgroups in an unsigned
int predict_check_size(const cn_engine* e, int n_steps, int n_modes, const char* who) {
    const uint64_t lanes = (uint64_t)e->P.B * (uint64_t)n_modes * (uint64_t)(e->P.A - 1);
    if (lanes > (uint64_t)INT32_MAX || (lanes > 0 && (uint64_t)n_steps > (uint64_t)INT32_MAX / lanes))
        return fail(CN_ERR_UNSUPPORTED, "%s: num_envs * n_modes * n_steps * num_humans = %llu * %d rows exceed the %llu a launch "
                    "indexes", who, (unsigned long long)lanes, n_steps, (unsigned long long)INT32_MAX);
    return CN_OK;
}

int run_predict(cn_engine* e, int n_steps, const Predict& pred, double* human_vel) {
    const cn::Params& P = e->P;
    hipLaunchKernelGGL(cn::predict_kernel, dim3(plan_grid((size_t)P.B * pred.n_modes * (P.A - 1))), dim3(cn::kPlanBlock), 0, e->stream,
                       P.B, P.A, pred.n_modes, n_steps, P.dt, pred.models, (const double2*)e->S.pos, (const double2*)e->S.vel,
                       (const double2*)e->S.goal, (const double2*)e->S.rv, (double2*)human_vel);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// cn_predict_orca's launch: step_kernel's grid, workgroup and LDS under the engine's Params with the robot out of the humans'
// sight and no ORCA robot (predict_orca_kernel.h); slot `mode` of the table.  robot_actions (cn_predict_orca_robot): the robot
// in their sight instead, whatever the engine's own setting — nothing of the workgroup's LDS, of the kd layout or of the
// geometry is sized by robot_visible — following rows env_stride apart; a unicycle's rows where the engine's step kernels
// would read them as such.
int run_predict_orca(cn_engine* e, int n_steps, int n_modes, int mode, double* human_vel, const double* robot_actions = nullptr,
                     int64_t env_stride = 0) {
    cn::Params Pk = e->P;
    Pk.robot_visible = robot_actions ? 1 : 0, Pk.robot_orca = 0;
    pick_maxl(e, [&](auto maxl) {
        pick_bool(Pk.kd != 0, [&](auto kd) {
            constexpr int kMaxl = decltype(maxl)::value;
            constexpr bool kKd = decltype(kd)::value;
            if (!robot_actions) {
                hipLaunchKernelGGL((cn::predict_orca_kernel<kMaxl, kKd>), dim3(grid_envs(e)), dim3(Pk.threads), e->smem, e->stream, Pk,
                                   e->S, n_steps, n_modes, mode, (double2*)human_vel);
                return;
            }
            pick_bool(e->P.robot_unicycle && !e->P.robot_orca, [&](auto uni) {
                hipLaunchKernelGGL((cn::predict_orca_robot_kernel<kMaxl, kKd, decltype(uni)::value>), dim3(grid_envs(e)),
                                   dim3(Pk.threads), e->smem, e->stream, Pk, e->S, n_steps, n_modes, mode, (double2*)human_vel,
                                   robot_actions, (long long)(env_stride ? env_stride : n_steps));
            });
        });
    });
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// cn_predict_orca_goals' launch: the same workgroup over B M virtual envs — the copy of Params counts them in B, so the grid,
// lane_of and build_pairs do; the kernel maps a virtual env back to its real one where it loads the agents
// (predict_orca_kernel.h).  E, the workgroup size and the LDS per workgroup are the engine's.
int run_predict_orca_goals(cn_engine* e, int n_steps, int n_modes, const double* goals, double* human_vel) {
    cn::Params Pk = e->P;
    Pk.B = e->P.B * n_modes, Pk.robot_visible = 0, Pk.robot_orca = 0;  // (within an int: predict_check_size)
    pick_maxl(e, [&](auto maxl) {
        pick_bool(Pk.kd != 0, [&](auto kd) {
            hipLaunchKernelGGL((cn::predict_orca_goals_kernel<decltype(maxl)::value, decltype(kd)::value>),
                               dim3(((unsigned)Pk.B + (unsigned)Pk.E - 1u) / (unsigned)Pk.E), dim3(Pk.threads), e->smem, e->stream, Pk, e->S, n_steps, n_modes,
                               (const double2*)goals, (double2*)human_vel);
        });
    });
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// The closed loop of either planner.  pred (the *_predict_rollout calls, whose checks of it precede this): every planning step
// scores against the table the device predictors make from the state as it then stands; orca_mode >= 0 (the
// *_predict_orca_rollout calls): slot orca_mode of that table is then overwritten by cn_predict_orca's.  nominal (the
// *_nominal_rollout calls): by cn_predict_orca_robot's instead, the robot on candidate 0 of the planning step's first draw — the
// plan's mean under the draw's clip rule; that draw is made ahead of the prediction and not again by run_plan.
int run_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                uint32_t counter, const char* who, const Mppi* mppi, const cn_predictors* pred = nullptr,
                const Predict& models = Predict{}, int orca_mode = -1, bool nominal = false) {
    int rc = plan_check(e, cfg, plan, who, mppi);
    if (rc || (rc = plan_check_io(e, io, plan))) return rc;
    if (n_real_steps < 0) return fail(CN_ERR_INVALID, "%s: n_real_steps must be >= 0 (got %d)", who, n_real_steps);
    // M == 1: the *_paths planner (bootstrap served); M > 1: the *_modes planner
    const bool many = pred && pred->n_modes > 1;
    const cn_path_modes modes{many ? pred->n_modes : 0, many ? pred->reduce : 0, many ? pred->risk_penalty : 0.0,
                              pred ? pred->human_vel : nullptr, many ? pred->weight : nullptr};
    if (many && (rc = plan_check_modes(e, cfg, plan, &modes, who))) return rc;
    if (pred && (rc = predict_check_size(e, cfg->n_steps, pred->n_modes, who))) return rc;
    for (int s = 0; s < n_real_steps; ++s) {
        if ((rc = bind(e)) || (pred && (rc = run_predict(e, cfg->n_steps, models, pred->human_vel)))) return rc;
        const uint32_t c = counter + (uint32_t)s * (uint32_t)cfg->iterations;
        if (nominal && (rc = run_draw(e, cfg, plan, c))) return rc;
        if (orca_mode >= 0 &&
            (rc = run_predict_orca(e, cfg->n_steps, pred->n_modes, orca_mode, pred->human_vel, nominal ? plan->candidates : nullptr,
                                   (int64_t)cfg->n_candidates * cfg->n_steps)))
            return rc;
        if ((rc = run_plan(e, cfg, plan, c, mppi, pred && !many ? pred->human_vel : nullptr, many ? &modes : nullptr, nominal)))
            return rc;
        if ((rc = cn_rollout_step(e, io, plan->action)) || (rc = run_shift(e, io, cfg, plan))) return rc;
    }
    return CN_OK;
}

// the checks of `pred` that come before everything else of a *_predict_rollout call
// (orca_mode: the *_predict_orca_rollout calls' argument, checked behind the models; NULL: the call has none)
int predict_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                    const cn_predictors* pred, uint32_t counter, const char* who, const Mppi* mppi, const int* orca_mode = nullptr,
                    bool nominal = false) {
    if (!pred) return fail(CN_ERR_INVALID, "%s: pred is NULL", who);
    if (!pred->human_vel) return fail(CN_ERR_INVALID, "%s: pred->human_vel is NULL", who);
    Predict models;
    const int rc = predict_check_models(pred->n_modes, pred->model, who, &models);
    if (rc) return rc;
    if (orca_mode && (*orca_mode < 0 || *orca_mode >= pred->n_modes))
        return fail(CN_ERR_INVALID, "%s: orca_mode = %d is outside 0 .. n_modes - 1 = %d", who, *orca_mode, pred->n_modes - 1);
    return run_rollout(e, io, n_real_steps, cfg, plan, counter, who, mppi, pred, models, orca_mode ? *orca_mode : -1, nominal);
}

// cn_predict_orca's checks, in the header's order, and the launch; robot_actions: cn_predict_orca_robot's, whose own checks came first
int predict_orca(cn_engine* e, int n_steps, int n_modes, int mode, double* human_vel, const char* who,
                 const double* robot_actions = nullptr, int64_t env_stride = 0) {
    if (!human_vel) return fail(CN_ERR_INVALID, "%s: human_vel is NULL", who);
    if (n_modes < 1) return fail(CN_ERR_INVALID, "%s: n_modes must be >= 1 (got %d)", who, n_modes);
    if (n_modes > cn::kPredictMaxModes)
        return fail(CN_ERR_UNSUPPORTED, "%s: n_modes = %d exceeds the %d modes of a table", who, n_modes, cn::kPredictMaxModes);
    if (mode < 0 || mode >= n_modes)
        return fail(CN_ERR_INVALID, "%s: mode = %d is outside 0 .. n_modes - 1 = %d", who, mode, n_modes - 1);
    if (n_steps < 0) return fail(CN_ERR_INVALID, "%s: n_steps must be >= 0 (got %d)", who, n_steps);
    if (!e) return fail(CN_ERR_INVALID, "%s: engine is NULL", who);
    int rc = predict_check_size(e, n_steps, n_modes, who);
    if (rc || n_steps == 0) return rc;
    if ((rc = bind(e))) return rc;
    return run_predict_orca(e, n_steps, n_modes, mode, human_vel, robot_actions, env_stride);
}

}  // namespace

extern "C" {

int cn_plan_set_unicycle(cn_engine* e, double max_rotation, double init_std_rotation) {
    if (!e) return fail(CN_ERR_INVALID, "cn_plan_set_unicycle: engine is NULL");
    if (!std::isfinite(max_rotation) || !(max_rotation > 0.0) || max_rotation > 3.141592653589793)
        return fail(CN_ERR_INVALID, "cn_plan_set_unicycle: max_rotation must be in (0, pi] (got %g)", max_rotation);
    if (!std::isfinite(init_std_rotation) || !(init_std_rotation > 0.0))
        return fail(CN_ERR_INVALID, "cn_plan_set_unicycle: init_std_rotation must be > 0 and finite (got %g)", init_std_rotation);
    if (!e->P.robot_unicycle || e->P.robot_orca)
        return fail(CN_ERR_INVALID, "cn_plan_set_unicycle is for CN_UNICYCLE engines with a CN_ROBOT_EXTERNAL robot: no other engine's "
                    "planner would read the setting");
    e->plan_max_rotation = max_rotation, e->plan_std_rotation = init_std_rotation;
    return CN_OK;
}

int cn_plan_get_unicycle(cn_engine* e, double* max_rotation, double* init_std_rotation) {
    if (!e) return fail(CN_ERR_INVALID, "cn_plan_get_unicycle: engine is NULL");
    if (!max_rotation || !init_std_rotation) return fail(CN_ERR_INVALID, "cn_plan_get_unicycle: an output is NULL");
    *max_rotation = e->plan_max_rotation, *init_std_rotation = e->plan_std_rotation;
    return CN_OK;
}

int cn_plan_reset(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const uint8_t* mask) {
    int rc = plan_check(e, cfg, plan, "cn_plan_reset");
    if (rc || (rc = bind(e))) return rc;
    return run_reset(e, cfg, plan, mask);
}

int cn_plan_draw(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter) {
    int rc = plan_check(e, cfg, plan, "cn_plan_draw");
    if (rc || (rc = bind(e))) return rc;
    return run_draw(e, cfg, plan, counter);
}

int cn_plan_refit(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, int keep_best) {
    int rc = plan_check(e, cfg, plan, "cn_plan_refit");
    if (rc || (rc = bind(e))) return rc;
    return run_refit(e, cfg, plan, keep_best);
}

int cn_plan_cem(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter) {
    int rc = plan_check(e, cfg, plan, "cn_plan_cem");
    if (rc || (rc = bind(e))) return rc;
    return run_plan(e, cfg, plan, counter, nullptr);
}

int cn_plan_shift(cn_engine* e, const cn_rollout_io* io, const cn_plan_cfg* cfg, const cn_plan* plan) {
    int rc = plan_check(e, cfg, plan, "cn_plan_shift");
    if (rc || (rc = plan_check_io(e, io, plan)) || (rc = bind(e))) return rc;
    return run_shift(e, io, cfg, plan);
}

int cn_plan_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                    uint32_t counter) {
    return run_rollout(e, io, n_real_steps, cfg, plan, counter, "cn_plan_rollout", nullptr);
}

int cn_plan_mppi_update(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, double temperature, int fit_std, int keep_best) {
    const Mppi mppi{temperature, fit_std};
    int rc = plan_check(e, cfg, plan, "cn_plan_mppi_update", &mppi);
    if (rc || (rc = bind(e))) return rc;
    return run_mppi_update(e, cfg, plan, mppi, keep_best);
}

int cn_plan_mppi(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, double temperature, int fit_std, uint32_t counter) {
    const Mppi mppi{temperature, fit_std};
    int rc = plan_check(e, cfg, plan, "cn_plan_mppi", &mppi);
    if (rc || (rc = bind(e))) return rc;
    return run_plan(e, cfg, plan, counter, &mppi);
}

int cn_plan_cem_paths(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const double* human_vel, uint32_t counter) {
    if (!human_vel) return fail(CN_ERR_INVALID, "cn_plan_cem_paths: human_vel is NULL");
    int rc = plan_check(e, cfg, plan, "cn_plan_cem_paths");
    if (rc || (rc = bind(e))) return rc;
    return run_plan(e, cfg, plan, counter, nullptr, human_vel);
}

int cn_plan_mppi_paths(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const double* human_vel, double temperature,
                       int fit_std, uint32_t counter) {
    if (!human_vel) return fail(CN_ERR_INVALID, "cn_plan_mppi_paths: human_vel is NULL");
    const Mppi mppi{temperature, fit_std};
    int rc = plan_check(e, cfg, plan, "cn_plan_mppi_paths", &mppi);
    if (rc || (rc = bind(e))) return rc;
    return run_plan(e, cfg, plan, counter, &mppi, human_vel);
}

int cn_plan_cem_modes(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const cn_path_modes* modes, uint32_t counter) {
    if (!modes) return fail(CN_ERR_INVALID, "cn_plan_cem_modes: modes is NULL");
    int rc = plan_check(e, cfg, plan, "cn_plan_cem_modes");
    if (rc || (rc = plan_check_modes(e, cfg, plan, modes, "cn_plan_cem_modes")) || (rc = bind(e))) return rc;
    return run_plan(e, cfg, plan, counter, nullptr, nullptr, modes);
}

int cn_plan_mppi_modes(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const cn_path_modes* modes, double temperature,
                       int fit_std, uint32_t counter) {
    if (!modes) return fail(CN_ERR_INVALID, "cn_plan_mppi_modes: modes is NULL");
    const Mppi mppi{temperature, fit_std};
    int rc = plan_check(e, cfg, plan, "cn_plan_mppi_modes", &mppi);
    if (rc || (rc = plan_check_modes(e, cfg, plan, modes, "cn_plan_mppi_modes")) || (rc = bind(e))) return rc;
    return run_plan(e, cfg, plan, counter, &mppi, nullptr, modes);
}

int cn_plan_mppi_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                         double temperature, int fit_std, uint32_t counter) {
    const Mppi mppi{temperature, fit_std};
    return run_rollout(e, io, n_real_steps, cfg, plan, counter, "cn_plan_mppi_rollout", &mppi);
}

int cn_predict(cn_engine* e, int n_steps, int n_modes, const int32_t* models, double* human_vel) {
    if (!models) return fail(CN_ERR_INVALID, "cn_predict: models is NULL");
    if (!human_vel) return fail(CN_ERR_INVALID, "cn_predict: human_vel is NULL");
    Predict pred;
    int rc = predict_check_models(n_modes, models, "cn_predict", &pred);
    if (rc) return rc;
    if (n_steps < 0) return fail(CN_ERR_INVALID, "cn_predict: n_steps must be >= 0 (got %d)", n_steps);
    if (!e) return fail(CN_ERR_INVALID, "cn_predict: engine is NULL");
    if ((rc = predict_check_size(e, n_steps, n_modes, "cn_predict")) || n_steps == 0) return rc;
    if ((rc = bind(e))) return rc;
    return run_predict(e, n_steps, pred, human_vel);
}

int cn_plan_cem_predict_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                                const cn_predictors* pred, uint32_t counter) {
    return predict_rollout(e, io, n_real_steps, cfg, plan, pred, counter, "cn_plan_cem_predict_rollout", nullptr);
}

int cn_plan_mppi_predict_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                                 const cn_predictors* pred, double temperature, int fit_std, uint32_t counter) {
    const Mppi mppi{temperature, fit_std};
    return predict_rollout(e, io, n_real_steps, cfg, plan, pred, counter, "cn_plan_mppi_predict_rollout", &mppi);
}

int cn_predict_orca(cn_engine* e, int n_steps, int n_modes, int mode, double* human_vel) {
    return predict_orca(e, n_steps, n_modes, mode, human_vel, "cn_predict_orca");
}

int cn_predict_orca_robot(cn_engine* e, int n_steps, int n_modes, int mode, const double* robot_actions, int64_t env_stride,
                          double* human_vel) {
    const char* who = "cn_predict_orca_robot";
    if (!human_vel) return fail(CN_ERR_INVALID, "%s: human_vel is NULL", who);
    if (!robot_actions) return fail(CN_ERR_INVALID, "%s: robot_actions is NULL", who);
    if (env_stride < 0 || (env_stride > 0 && env_stride < (int64_t)n_steps))
        return fail(CN_ERR_INVALID, "%s: env_stride = %lld rows must be 0 (= n_steps) or >= n_steps = %d", who, (long long)env_stride,
                    n_steps);
    return predict_orca(e, n_steps, n_modes, mode, human_vel, who, robot_actions, env_stride);
}

int cn_plan_cem_predict_orca_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                     const cn_plan* plan, const cn_predictors* pred, int orca_mode, uint32_t counter) {
    return predict_rollout(e, io, n_real_steps, cfg, plan, pred, counter, "cn_plan_cem_predict_orca_rollout", nullptr, &orca_mode);
}

int cn_plan_mppi_predict_orca_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                      const cn_plan* plan, const cn_predictors* pred, int orca_mode, double temperature, int fit_std,
                                      uint32_t counter) {
    const Mppi mppi{temperature, fit_std};
    return predict_rollout(e, io, n_real_steps, cfg, plan, pred, counter, "cn_plan_mppi_predict_orca_rollout", &mppi, &orca_mode);
}

int cn_plan_cem_predict_orca_nominal_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                             const cn_plan* plan, const cn_predictors* pred, int orca_mode, uint32_t counter) {
    return predict_rollout(e, io, n_real_steps, cfg, plan, pred, counter, "cn_plan_cem_predict_orca_nominal_rollout", nullptr, &orca_mode,
                           true);
}

int cn_plan_mppi_predict_orca_nominal_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                              const cn_plan* plan, const cn_predictors* pred, int orca_mode, double temperature,
                                              int fit_std, uint32_t counter) {
    const Mppi mppi{temperature, fit_std};
    return predict_rollout(e, io, n_real_steps, cfg, plan, pred, counter, "cn_plan_mppi_predict_orca_nominal_rollout", &mppi, &orca_mode,
                           true);
}

int cn_predict_orca_goals(cn_engine* e, int n_steps, int n_modes, const double* goals, double* human_vel) {
    const char* who = "cn_predict_orca_goals";
    if (!goals) return fail(CN_ERR_INVALID, "%s: goals is NULL", who);
    if (!human_vel) return fail(CN_ERR_INVALID, "%s: human_vel is NULL", who);
    if (n_modes < 1) return fail(CN_ERR_INVALID, "%s: n_modes must be >= 1 (got %d)", who, n_modes);
    if (n_modes > cn::kPredictMaxModes)
        return fail(CN_ERR_UNSUPPORTED, "%s: n_modes = %d exceeds the %d modes of a table", who, n_modes, cn::kPredictMaxModes);
    if (n_steps < 0) return fail(CN_ERR_INVALID, "%s: n_steps must be >= 0 (got %d)", who, n_steps);
    if (!e) return fail(CN_ERR_INVALID, "%s: engine is NULL", who);
    int rc = predict_check_size(e, n_steps, n_modes, who);  // (B M <= B M (A - 1): the virtual envs are within an int as well)
    if (rc || n_steps == 0) return rc;
    if ((rc = bind(e))) return rc;
    return run_predict_orca_goals(e, n_steps, n_modes, goals, human_vel);
}

int cn_goal_hypotheses(cn_engine* e, int n_modes, int base, double reach, double std_heading, double std_distance, int nominal_first,
                       uint64_t seed, uint32_t counter, double* goals) {
    const char* who = "cn_goal_hypotheses";
    if (!goals) return fail(CN_ERR_INVALID, "%s: goals is NULL", who);
    if (n_modes < 1) return fail(CN_ERR_INVALID, "%s: n_modes must be >= 1 (got %d)", who, n_modes);
    if (n_modes > cn::kPredictMaxModes)
        return fail(CN_ERR_UNSUPPORTED, "%s: n_modes = %d exceeds the %d modes of a table", who, n_modes, cn::kPredictMaxModes);
    if (base != CN_GOALS_ENGINE && base != CN_GOALS_HEADING)
        return fail(CN_ERR_INVALID, "%s: base = %d unknown (CN_GOALS_ENGINE = 0, CN_GOALS_HEADING = 1)", who, base);
    if (base == CN_GOALS_HEADING && (!std::isfinite(reach) || !(reach > 0.0)))
        return fail(CN_ERR_INVALID, "%s: reach must be > 0 and finite under CN_GOALS_HEADING (got %g)", who, reach);
    if (!std::isfinite(std_heading) || !(std_heading >= 0.0))
        return fail(CN_ERR_INVALID, "%s: std_heading must be >= 0 and finite (got %g)", who, std_heading);
    if (!std::isfinite(std_distance) || !(std_distance >= 0.0))
        return fail(CN_ERR_INVALID, "%s: std_distance must be >= 0 and finite (got %g)", who, std_distance);
    if (!e) return fail(CN_ERR_INVALID, "%s: engine is NULL", who);
    int rc = predict_check_size(e, 1, n_modes, who);  // (the grid counts workgroups in an unsigned)
    if (rc || (rc = bind(e))) return rc;
    const cn::Params& P = e->P;
    hipLaunchKernelGGL(cn::goal_hypotheses_kernel, dim3(plan_grid((size_t)P.B * n_modes * (P.A - 1))), dim3(cn::kPlanBlock), 0, e->stream,
                       P.B, P.A, n_modes, base == CN_GOALS_HEADING ? 1 : 0, nominal_first ? 1 : 0, reach, std_heading, std_distance,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), counter, (const double2*)e->S.pos,
                       (const double2*)e->S.vel, (const double2*)e->S.goal, (double2*)goals);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

}  // extern "C"
