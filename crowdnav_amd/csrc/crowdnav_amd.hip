// libcrowdnav_amd.so — the C ABI declared in include/crowdnav_amd.h over the HIP kernels of step_kernels.h, scenario_ring.h,
// rollout_kernels.h and rollout_fused.h.
//
// Hot path replaced (reference file:line, /root/reference):
//   CrowdSim.step / onestep_lookahead          crowd_sim/envs/crowd_sim.py:314-420
//   Human.act / Robot.act -> ORCA.predict      crowd_sim/envs/utils/human.py:9-17, policy/orca.py:82-132
//   rvo2 doStep (un-vendored RVO2 library)     orca.py:128
//   Agent.compute_position / step              crowd_sim/envs/utils/agent.py:110-135
//   point_to_segment_dist                      crowd_sim/envs/utils/utils.py:4-26
//   CrowdSim.reset + scenario rules            crowd_sim.py:155-207, 251-312
//   Explorer.run_k_episodes inner loop         crowd_nav/utils/explorer.py:35-72
//
// Built with -ffp-contract=off: float32 ORCA and float64 env arithmetic must round exactly like the CPU
// reference; the only fused operation is the explicit fma in norm2().
#include "engine_host.h"
#include "scenario_ring_host.h"
#include "rollout_fused.h"
#include "records_kernels.h"
#include "lookahead_cv_kernel.h"
#include "lookahead_modes_kernel.h"

thread_local char cn_g_err[512] = "";

// every agent's ORCA velocity on the engine's stream (cn_orca; the first kernel of cn_sarl_select in sarl_abi.hip)
void cn_launch_orca(cn_engine* e, float* out_vel) {
    pick_maxl(e, [&](auto maxl) {
        pick_bool(e->P.kd, [&](auto kd) {
            hipLaunchKernelGGL((cn::orca_kernel<decltype(maxl)::value, decltype(kd)::value>), dim3(grid_envs(e)), dim3(e->P.threads),
                               e->smem, e->stream, e->P, e->S, out_vel);
        });
    });
}

// BASELINE configs[1]: 5 humans + robot, 2 envs per workgroup — the geometry the fused kernels hold as compile-time constants
static bool headline_geometry(const cn::Params& P) {
    return P.A == 6 && P.NC == 5 && P.E == 2 && P.nA == 12 && P.pairs == 60 && P.threads == 64;
}

// the two-wave kernel's and the one-wave kernels' instantiations of rollout_fused_kernel: f(kernel, threads per workgroup) for
// the one a route of this engine runs (CN_ROUTE_FUSED_SPLIT or CN_ROUTE_FUSED) — the launch and the occupancy query name it HERE
template <class F>
static void pick_fused(const cn_engine* e, int route, F&& f) {
    if (route == CN_ROUTE_FUSED_SPLIT) {
        if (e->split_assist & cn::kAssistHead) f(cn::rollout_fused_kernel<true, true, cn::kAssistHead>, 2 * cn::kWave);
        else f(cn::rollout_fused_kernel<true, true>, 2 * cn::kWave);
    } else if (headline_geometry(e->P)) {
        f(cn::rollout_fused_kernel<true>, cn::kWave);
    } else {
        f(cn::rollout_fused_kernel<false>, cn::kWave);
    }
}

// cn_lookahead_actions' refusals, which cn_lookahead_values (sarl_abi.hip) makes first as well, with these messages: what depends
// on the arguments alone, then what depends on the engine
int cn_lookahead_check(const cn_engine* e, int n_steps, int n_candidates, const double* actions, const cn_lookahead_out* out) {
    if (!actions) return fail(CN_ERR_INVALID, "cn_lookahead_actions: actions is NULL");
    if (!out) return fail(CN_ERR_INVALID, "cn_lookahead_actions: out is NULL");
    if (!out->ret) return fail(CN_ERR_INVALID, "cn_lookahead_actions: out->ret is NULL");
    if (!out->info) return fail(CN_ERR_INVALID, "cn_lookahead_actions: out->info is NULL");
    if (!out->steps) return fail(CN_ERR_INVALID, "cn_lookahead_actions: out->steps is NULL");
    if (!out->time) return fail(CN_ERR_INVALID, "cn_lookahead_actions: out->time is NULL");
    if (n_steps < 0) return fail(CN_ERR_INVALID, "cn_lookahead_actions: n_steps must be >= 0 (got %d)", n_steps);
    if (n_candidates < 1) return fail(CN_ERR_INVALID, "cn_lookahead_actions: n_candidates must be >= 1 (got %d)", n_candidates);
    if (!e) return fail(CN_ERR_INVALID, "cn_lookahead_actions: engine is NULL");
    if (e->P.robot_orca)
        return fail(CN_ERR_INVALID, "cn_lookahead_actions is for CN_ROBOT_EXTERNAL engines (an ORCA robot takes no actions)");
    // the virtual env index is an int (Lane::env; a workgroup's last lanes may look E - 1 past the end), rows are size_t
    const uint64_t virtual_envs = (uint64_t)e->P.B * (uint64_t)n_candidates, rows = virtual_envs * (uint64_t)n_steps;
    if (virtual_envs > (uint64_t)INT32_MAX - cn::kWave)
        return fail(CN_ERR_UNSUPPORTED, "cn_lookahead_actions: num_envs * n_candidates = %llu exceeds the %llu branches a launch "
                    "indexes", (unsigned long long)virtual_envs, (unsigned long long)((uint64_t)INT32_MAX - cn::kWave));
    if (rows > ((uint64_t)1 << 59))
        return fail(CN_ERR_UNSUPPORTED, "cn_lookahead_actions: num_envs * n_candidates * n_steps = %llu action rows exceed 2^59",
                    (unsigned long long)rows);
    if (!e->discount || e->discount_len <= 0)
        return fail(CN_ERR_INVALID, "cn_lookahead_actions: the engine has no discount table (cn_set_gamma)");
    return CN_OK;
}

// the device copy of a lookahead's cn_lookahead_out: uploaded when it differs from the last one (ordered on the engine's
// stream, as upload_io)
static int upload_look(cn_engine* e, const cn_lookahead_out* out) {
    if (!e->look_valid || std::memcmp(&e->look_host, out, sizeof(*out)) != 0) {
        e->look_host = *out;
        CN_HIP(hipMemcpyAsync(e->look_dev, &e->look_host, sizeof(*out), hipMemcpyHostToDevice, e->stream));
        e->look_valid = true;
    }
    return CN_OK;
}

// ... and the engine's goal weight behind it, where rollout_lookahead_goal_kernel reads it: uploaded by the launch that needs it
// when it differs from the last one, likewise (the setter itself touches nothing on the device)
static int upload_look_goal(cn_engine* e) {
    if (e->look_goal_dev != e->look_goal_weight) {
        e->look_goal_dev = e->look_goal_weight;
        CN_HIP(hipMemcpyAsync(e->look_dev + 1, &e->look_goal_dev, sizeof(double), hipMemcpyHostToDevice, e->stream));
    }
    return CN_OK;
}

// what lookahead_cv_kernel and lookahead_paths_kernel read of the engine
static cn::CvParams cv_params(const cn_engine* e, int n_steps, int n_candidates) {
    const cn::Params& P = e->P;
    cn::CvParams C{};
    C.B = P.B, C.K = n_candidates, C.A = P.A, C.n_steps = n_steps;
    C.chunks = (n_candidates + cn::kWave - 1) / cn::kWave;
    C.discount_len = e->discount_len, C.discount = e->discount;
    C.dt = P.dt, C.time_limit = P.time_limit, C.success_reward = P.success_reward, C.collision_penalty = P.collision_penalty;
    C.discomfort_dist = P.discomfort_dist, C.discomfort_factor = P.discomfort_factor;
    C.pos = e->S.pos, C.vel = e->S.vel, C.goal = e->S.goal, C.rv = e->S.rv, C.gtime = e->S.gtime, C.theta = e->S.theta;
    return C;
}

extern "C" {

const char* cn_last_error(void) { return cn_g_err; }
int cn_abi_version(void) { return CN_ABI_VERSION; }

static int check_config(const cn_config* c) {
    if (c->num_envs < 1) return fail(CN_ERR_INVALID, "num_envs must be >= 1 (got %d)", c->num_envs);
    if (c->num_humans < 1 || c->num_humans > 63)
        return fail(CN_ERR_UNSUPPORTED, "num_humans must be in 1..63 (got %d)", c->num_humans);
    if (c->max_neighbors < 0 || c->max_neighbors > cn::kMaxNb)
        return fail(CN_ERR_UNSUPPORTED, "max_neighbors must be in 0..%d (got %d)", cn::kMaxNb, c->max_neighbors);
    if (!(c->time_step > 0.0)) return fail(CN_ERR_INVALID, "time_step must be > 0");
    if (c->scenario_rule != CN_CIRCLE_CROSSING && c->scenario_rule != CN_SQUARE_CROSSING && c->scenario_rule != CN_MIXED)
        return fail(CN_ERR_UNSUPPORTED, "scenario_rule %d not supported", c->scenario_rule);
    if (c->scenario_rule == CN_MIXED) {
        if (c->num_humans < 5 || c->num_humans > 8)
            return fail(CN_ERR_UNSUPPORTED, "scenario_rule mixed draws up to 5 humans per episode: num_humans must be in 5..8 (got %d)",
                        c->num_humans);
        if (c->randomize_attributes && c->robot_policy == CN_ROBOT_ORCA)
            return fail(CN_ERR_UNSUPPORTED,
                        "mixed + randomize_attributes + the ORCA robot: the reference rebuilds the robot's rvo2 simulator "
                        "whenever the number of humans changes (orca.py:95-98), which the per-env radius capture does not model");
    }
    if (c->robot_policy != CN_ROBOT_EXTERNAL && c->robot_policy != CN_ROBOT_ORCA)
        return fail(CN_ERR_INVALID, "robot_policy %d unknown", c->robot_policy);
    if (c->robot_kinematics != CN_HOLONOMIC && c->robot_kinematics != CN_UNICYCLE)
        return fail(CN_ERR_INVALID, "robot_kinematics %d unknown", c->robot_kinematics);
    if (c->robot_kinematics == CN_UNICYCLE && c->robot_policy == CN_ROBOT_ORCA)
        return fail(CN_ERR_INVALID, "the ORCA robot policy is holonomic (orca.py:59); a unicycle robot needs CN_ROBOT_EXTERNAL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(CN_ERR_NO_DEVICE, "no HIP device visible: the MI355X engine has no CPU fallback");
    if (c->device < 0 || c->device >= ndev) return fail(CN_ERR_INVALID, "device %d out of range", c->device);
    return CN_OK;
}

// what the kernels and the scenario generators take from the caller's configuration as it stands
static void copy_config(cn_engine* e) {
    const cn_config* c = &e->cfg;
    cn::Params& P = e->P;
    P.robot_visible = c->robot_visible ? 1 : 0;
    P.robot_orca = c->robot_policy == CN_ROBOT_ORCA;
    P.robot_unicycle = c->robot_kinematics == CN_UNICYCLE;
    P.dt = c->time_step;
    P.time_limit = c->time_limit;
    P.success_reward = c->success_reward;
    P.collision_penalty = c->collision_penalty;
    P.discomfort_dist = c->discomfort_dist;
    P.discomfort_factor = c->discomfort_penalty_factor;
    P.robot_safety = c->robot_safety_space;
    P.human_safety = c->human_safety_space;
    P.orca.neighbor_dist = (float)c->neighbor_dist;
    P.orca.inv_time_horizon = 1.0f / (float)c->time_horizon;
    P.orca.inv_time_step = 1.0f / (float)c->time_step;
    P.orca.max_neighbors = c->max_neighbors;
    e->C.num_agents = c->num_humans + 1;
    e->C.rule = c->scenario_rule;
    e->C.randomize = c->randomize_attributes ? 1 : 0;
    e->C.circle_radius = c->circle_radius;
    e->C.square_width = c->square_width;
    e->C.discomfort_dist = c->discomfort_dist;
    e->C.human_radius = c->human_radius;
    e->C.human_v_pref = c->human_v_pref;
    e->C.robot_radius = c->robot_radius;
    e->C.robot_v_pref = c->robot_v_pref;
}

// Workgroup geometry.  E envs per workgroup (agents = lanes of wave 0), W waves sharing the per-pair phases.
// Defaults from the MI355X sweep in DESIGN.md; CROWDNAV_AMD_ENVS_PER_WAVE / CROWDNAV_AMD_WAVES_PER_BLOCK
// override them for tuning.
static void pick_geometry(cn_engine* e) {
    const cn_config* c = &e->cfg;
    cn::Params& P = e->P;
    P.B = c->num_envs;
    P.A = c->num_humans + 1;
    P.NC = P.A - 1;
    const int e_max = cn::kWave / P.A;
    // <= 5 half-planes per agent: 2048 workgroups (2 waves per SIMD) were fastest; the 10-half-plane kernels hold
    // 187 VGPRs (2 resident waves per SIMD) and loop over many more pairs, so they get one env per wave up to
    // 4096 workgroups (H = 20: E = 1 48 M, E = 2 31 M env-steps/s)
    const bool small_lp = (P.NC < c->max_neighbors ? P.NC : c->max_neighbors) <= 5;
    // (r02, candidate-form programs: their (agent, half-plane) items fill one 64-lane pass at 2 envs x 6 agents; E = 3..8
    // take 2-3 passes and lose 25-45 % at 8192-32768 envs, so the small programs never pack more than 2 envs per wave)
    int e_want = env_int("CROWDNAV_AMD_ENVS_PER_WAVE", small_lp ? (P.B > 2048 ? 2 : 1) : (P.B + 4095) / 4096);
    P.E = e_want < 1 ? 1 : (e_want > e_max ? e_max : e_want);
    int w_want = env_int("CROWDNAV_AMD_WAVES_PER_BLOCK", 1);
    const int w_useful = (P.E * P.A * P.NC + cn::kWave - 1) / cn::kWave;  // more waves than pair passes is waste
    if (w_want > w_useful) w_want = w_useful;
    if (w_want > cn::kMaxBlock / cn::kWave) w_want = cn::kMaxBlock / cn::kWave;
    P.threads = cn::kWave * (w_want < 1 ? 1 : w_want);
    P.nA = P.E * P.A;
    P.pairs = P.nA * P.NC;
    e->maxl = small_lp ? 5 : 10;
    P.kd = P.A > cn::kKdLeaf ? 1 : 0;  // a simulator of more than 10 agents splits its kd-tree: visiting order matters at ties
    P.kdl = cn::kd_layout(P.nA, P.A, P.E);
    e->smem = cn::smem_bytes(P.nA, P.pairs, e->maxl, P.A, P.E);
}

static int rollout_route(const cn_engine* e, const double* action);

// The run-time switches and what they are weighed against: the device's size.  The scenario ring reads its own.
static void read_knobs(cn_engine* e) {
    const cn_config* c = &e->cfg;
    cn::Params& P = e->P;
    P.sched = -1;
    e->sched_min = env_int("CROWDNAV_AMD_SCHED_MIN_STEPS", 24);  // shortest call that runs under a schedule (static: at least 48)
    e->sched_force = env_int("CROWDNAV_AMD_SCHED_FORCE", 0) != 0;
    e->sched_reserve = env_int("CROWDNAV_AMD_DYN_RESERVE", 0);  // slots left free beside a dynamic launch under the asynchronous fill
    e->sched_dynamic = env_int("CROWDNAV_AMD_SCHED_DYNAMIC", 1) != 0;
    e->dyn_visits = env_int("CROWDNAV_AMD_DYN_VISITS", 0);  // 0: by call length (launch_shard)
    P.dyn_visits = 3;
    e->use_fused = env_int("CROWDNAV_AMD_FUSED", 1) != 0;
    // 0: the one-wave fused kernel everywhere (A/B runs); 2: the two-wave kernel also for launches of several rounds (measurements)
    e->fused_split = env_int("CROWDNAV_AMD_FUSED_SPLIT", 1);
    // what the env wave of the two-wave kernel takes off the ORCA wave's chain (rollout_fused.h: ASSIST): 1 (default) = the head
    // of the 3-D fallback for the agents predicted infeasible; 0 = nothing (A/B runs)
    e->split_assist = env_int("CROWDNAV_AMD_SPLIT_ASSIST", 1) != 0 ? cn::kAssistHead : 0;
    // give-up threshold of the rejection sampling: ~seconds of GPU time in either generator family
    int cap_log2 = env_int("CROWDNAV_AMD_MAX_ATTEMPTS_LOG2", c->num_humans > 8 ? 23 : 20);
    if (cap_log2 < 6) cap_log2 = 6;
    if (cap_log2 > 40) cap_log2 = 40;
    e->C.max_attempts = 1ull << cap_log2;
    hipDeviceProp_t prop;
    const bool ok = hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0;
    e->sched_slots = 12 * (ok ? prop.multiProcessorCount : 256);
    e->ring.configure(e, ok ? prop.multiProcessorCount : 256);
    e->split_slots = 0;
    if (ok && headline_geometry(P))  // the two-wave kernel is for launches that fit the device in one round (rollout_route)
        pick_fused(e, CN_ROUTE_FUSED_SPLIT, [&](auto kernel, int threads) {
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, e->smem) == hipSuccess)
                e->split_slots = per_cu * prop.multiProcessorCount;
        });
    // the engines whose cn_rollout runs the two-wave kernel solve every ring scenario's first step when the slot is filled
    e->ring.first_step = rollout_route(e, nullptr) == CN_ROUTE_FUSED_SPLIT;
}

// every device buffer of the engine — the scenario ring allocates its own — and the device copy of the state view (the caller
// destroys the engine if this fails)
static int alloc_state(cn_engine* e) {
    const cn::Params& P = e->P;
    const size_t n = (size_t)P.B * P.A;
    int rc = CN_OK;
    cn::StateView& S = e->S;
    if ((rc = dev_alloc(e, &S.pos, n)) || (rc = dev_alloc(e, &S.vel, n)) || (rc = dev_alloc(e, &S.goal, n)) ||
        (rc = dev_alloc(e, &S.rv, n)) || (rc = dev_alloc(e, &S.gtime, (size_t)P.B)) ||
        (rc = dev_alloc(e, &S.theta, (size_t)P.B)) ||
        (rc = dev_alloc(e, &S.rsim_radius, n)) || (rc = dev_alloc(e, &S.rsim_max_speed, (size_t)P.B)) ||
        (rc = dev_alloc(e, &S.rsim_valid, (size_t)P.B)) || (rc = dev_alloc(e, &S.mt_key, (size_t)624 * P.B)) ||
        (rc = dev_alloc(e, &S.mt_pos, (size_t)P.B)) || (rc = dev_alloc(e, &e->probe_key, (size_t)624)) ||
        (rc = e->ring.create(e)) ||
        (rc = dev_alloc(e, &e->summary_scratch, (size_t)cn::kSummaryBlocks * cn::kSummaryFields + 1)) ||
        (rc = dev_alloc(e, &S.ep_word, (size_t)P.B)) || (rc = dev_alloc(e, &S.dyn_queue, (size_t)P.B + 1)) ||
        (rc = dev_alloc(e, &S.kd_order, P.kd ? n * cn::kd_row_bytes(P.A) : (size_t)4)) ||
        (rc = dev_alloc(e, &S.kd_valid, P.kd ? n : (size_t)4)) ||
        (rc = dev_alloc(e, &S.wg_partial, (size_t)P.B * (CN_SUMMARY_FIELDS + 1))) ||
        (rc = dev_alloc(e, &S.group_partial, (size_t)cn::kEpilogueGroups * (CN_SUMMARY_FIELDS + 1))) ||
        (rc = dev_alloc(e, &S.tickets, (size_t)(cn::kEpilogueGroups + 1) * cn::kTicketStride)) ||
        (rc = dev_alloc(e, &e->io_dev, (size_t)1)) || (rc = dev_alloc(e, &e->C.error, (size_t)1)) ||
        (rc = dev_alloc(e, &e->S_dev, (size_t)1)) || (rc = dev_alloc(e, &e->look_dev, (size_t)2)))
        return rc;
    e->S.error = e->C.error;
    if (hipMemcpy(e->S_dev, &e->S, sizeof(cn::StateView), hipMemcpyHostToDevice) != hipSuccess)
        return fail(CN_ERR_HIP, "cn_create: state view upload failed");
    return CN_OK;
}

int cn_create(const cn_config* c, cn_engine** out) {
    if (!c || !out) return fail(CN_ERR_INVALID, "cn_create: NULL argument");
    *out = nullptr;
    int rc = check_config(c);
    if (rc) return rc;
    CN_HIP(hipSetDevice(c->device));

    cn_engine* e = new (std::nothrow) cn_engine();
    if (!e) return fail(CN_ERR_INVALID, "out of host memory");
    e->cfg = *c;
    copy_config(e);
    pick_geometry(e);
    read_knobs(e);
    if ((rc = alloc_state(e)) || (rc = cn_set_gamma(e, 0.9))) {
        cn_destroy(e);
        return rc;
    }
    *out = e;
    return CN_OK;
}

int cn_destroy(cn_engine* e) {
    if (!e) return CN_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipStreamSynchronize(e->stream);
    e->ring.destroy();
    e->alloc_rollback(cn_engine::AllocMark{});
    if (e->discount) (void)hipFree(e->discount);
    cn_sarl_release(e);
    delete e;
    return CN_OK;
}

int cn_set_stream(cn_engine* e, void* hip_stream) {
    if (!e) return fail(CN_ERR_INVALID, "engine is NULL");
    e->stream = static_cast<hipStream_t>(hip_stream);
    e->orca_fresh = false;
    return CN_OK;
}

int cn_sync(cn_engine* e) {
    int rc = bind(e);
    if (rc) return rc;
    CN_HIP(hipStreamSynchronize(e->stream));
    if ((rc = e->ring.drain(e))) return rc;
    int gen_error = 0;
    CN_HIP(hipMemcpy(&gen_error, e->C.error, sizeof(int), hipMemcpyDeviceToHost));
    if (gen_error) {
        CN_HIP(hipMemset(e->C.error, 0, sizeof(int)));
        if (gen_error & 4)
            return fail(CN_ERR_HIP,
                        "the shard kernel's dynamic schedule: a workgroup waited ~2 s for an env's previous visit and went on "
                        "without it (results of this rollout are not to be trusted); CROWDNAV_AMD_SCHED_DYNAMIC=0 selects the "
                        "static schedule");
        if (gen_error & 2)
            return fail(CN_ERR_INVALID,
                        "cn_sarl_explore needs each env's numpy stream: (re)start the episodes with cn_reset (the scenario "
                        "ring of cn_rollout_* and the wave generator used for more than 8 humans do not keep it)");
        return fail(CN_ERR_INVALID,
                    "scenario generation gave up on a human after %llu rejected placements (the reference's rejection "
                    "sampling would not have terminated either: too many humans for this circle/square); the affected "
                    "scenario holds an overlapping placement",
                    e->C.max_attempts);
    }
    return CN_OK;
}

namespace {

__global__ void pack_state_kernel(int n, const double* state8, cn::StateView S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* s = state8 + (size_t)i * 8;
    S.pos[i] = make_double2(s[0], s[1]);
    S.vel[i] = make_double2(s[2], s[3]);
    S.goal[i] = make_double2(s[4], s[5]);
    S.rv[i] = make_double2(s[6], s[7]);
}

__global__ void unpack_state_kernel(int n, double* state8, cn::StateView S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double* s = state8 + (size_t)i * 8;
    const double2 p = S.pos[i], v = S.vel[i], g = S.goal[i], q = S.rv[i];
    s[0] = p.x, s[1] = p.y, s[2] = v.x, s[3] = v.y, s[4] = g.x, s[5] = g.y, s[6] = q.x, s[7] = q.y;
}

}  // namespace

int cn_set_state(cn_engine* e, const double* state8, const double* global_time) {
    int rc = bind(e);
    if (rc || (rc = e->ring.settle(e)) || (rc = e->ring.forget_first_steps(e))) return rc;
    const int n = e->P.B * e->P.A;
    if (state8) hipLaunchKernelGGL(pack_state_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, state8, e->S);
    if (global_time)
        CN_HIP(hipMemcpyAsync(e->S.gtime, global_time, sizeof(double) * e->P.B, hipMemcpyDeviceToDevice, e->stream));
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_get_state(cn_engine* e, double* state8, double* global_time) {
    int rc = bind(e);
    if (rc || (rc = e->ring.settle(e))) return rc;
    const int n = e->P.B * e->P.A;
    if (state8) hipLaunchKernelGGL(unpack_state_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, state8, e->S);
    if (global_time)
        CN_HIP(hipMemcpyAsync(global_time, e->S.gtime, sizeof(double) * e->P.B, hipMemcpyDeviceToDevice, e->stream));
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_set_theta(cn_engine* e, const double* theta) {
    int rc = bind(e);
    if (rc) return rc;
    if (!theta) return fail(CN_ERR_INVALID, "cn_set_theta: NULL");
    CN_HIP(hipMemcpyAsync(e->S.theta, theta, sizeof(double) * e->P.B, hipMemcpyDeviceToDevice, e->stream));
    return CN_OK;
}

int cn_get_theta(cn_engine* e, double* theta) {
    int rc = bind(e);
    if (rc) return rc;
    if (!theta) return fail(CN_ERR_INVALID, "cn_get_theta: NULL");
    CN_HIP(hipMemcpyAsync(theta, e->S.theta, sizeof(double) * e->P.B, hipMemcpyDeviceToDevice, e->stream));
    return CN_OK;
}

namespace {
__global__ void human_count_kernel(int B, int A, const double2* pos, int32_t* out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = 0;
    for (int i = 1; i < A; ++i) n += cn::is_parked(pos[(size_t)b * A + i]) ? 0 : 1;
    out[b] = n;
}
}  // namespace

int cn_get_human_count(cn_engine* e, int32_t* count) {
    int rc = bind(e);
    if (rc) return rc;
    if (!count) return fail(CN_ERR_INVALID, "cn_get_human_count: NULL");
    hipLaunchKernelGGL(human_count_kernel, dim3((e->P.B + 255) / 256), dim3(256), 0, e->stream, e->P.B, e->P.A, e->S.pos, count);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

namespace {
__global__ void set_robot_sim_kernel(int B, int A, const float* radii, float max_speed, cn::StateView S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * A) return;
    S.rsim_radius[i] = radii[i % A];
    if (i % A == 0) {
        S.rsim_max_speed[i / A] = max_speed;
        S.rsim_valid[i / A] = 1;
    }
}
}  // namespace

int cn_set_robot_sim(cn_engine* e, const float* radii_host, float max_speed) {
    int rc = bind(e);
    if (rc) return rc;
    if (!radii_host) return fail(CN_ERR_INVALID, "cn_set_robot_sim: NULL");
    // (a fill beside the previous launch may be solving first steps with the simulator as it was)
    if ((rc = e->ring.settle(e)) || (rc = e->ring.forget_first_steps(e))) return rc;
    e->ring.robot_sim_known = true;
    float* staged = reinterpret_cast<float*>(e->probe_key);  // 624 words of scratch, A <= 64
    CN_HIP(hipMemcpyAsync(staged, radii_host, sizeof(float) * e->P.A, hipMemcpyHostToDevice, e->stream));
    CN_HIP(hipStreamSynchronize(e->stream));  // radii_host may be a temporary
    hipLaunchKernelGGL(set_robot_sim_kernel, dim3((e->P.B * e->P.A + 255) / 256), dim3(256), 0, e->stream, e->P.B, e->P.A,
                       staged, max_speed, e->S);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_drop_robot_sim(cn_engine* e) {
    int rc = bind(e);
    if (rc || (rc = e->ring.settle(e)) || (rc = e->ring.forget_first_steps(e))) return rc;
    e->ring.robot_sim_known = false;
    CN_HIP(hipMemsetAsync(e->S.rsim_valid, 0, (size_t)e->P.B, e->stream));
    if (e->P.kd)  // ... and its simulator's kd-tree order: byte 0 of every env's A flags
        CN_HIP(hipMemset2DAsync(e->S.kd_valid, (size_t)e->P.A, 0, 1, (size_t)e->P.B, e->stream));
    return CN_OK;
}

int cn_drop_sims(cn_engine* e) {
    int rc = cn_drop_robot_sim(e);
    if (rc) return rc;
    if (e->P.kd) CN_HIP(hipMemsetAsync(e->S.kd_valid, 0, (size_t)e->P.B * e->P.A, e->stream));
    return CN_OK;
}

int cn_reset(cn_engine* e, const uint32_t* seeds, const uint8_t* mask, uint64_t* draws) {
    int rc = bind(e);
    if (rc || (rc = e->ring.settle(e))) return rc;
    if (!seeds) return fail(CN_ERR_INVALID, "cn_reset: seeds is NULL");
    if ((rc = e->ring.forget_first_steps(e))) return rc;
    if (e->ring.gen_wave)
        hipLaunchKernelGGL(cn::reset_wave_kernel, dim3(e->P.B), dim3(cn::kWave), 0, e->stream, e->P, e->C, e->S, seeds, mask,
                           draws);
    else
        hipLaunchKernelGGL(cn::reset_kernel, dim3(grid_lanes(e)), dim3(cn::kWave), 0, e->stream, e->P, e->C, e->S, seeds, mask,
                           draws);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_orca(cn_engine* e, float* out_vel) {
    int rc = bind(e);
    if (rc) return rc;
    if (!out_vel) return fail(CN_ERR_INVALID, "cn_orca: out_vel is NULL");
    cn_launch_orca(e, out_vel);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_step(cn_engine* e, const double* action, int update, double* reward, uint8_t* done, uint8_t* info,
            double* dmin, double* action_out, float* orca_vel, double* obs) {
    int rc = bind(e);
    if (rc || (rc = e->ring.settle(e))) return rc;
    if (!reward || !done || !info) return fail(CN_ERR_INVALID, "cn_step: reward/done/info must not be NULL");
    if (e->P.robot_orca && action)
        return fail(CN_ERR_INVALID, "cn_step: action must be NULL when robot_policy == CN_ROBOT_ORCA");
    if (!e->P.robot_orca && !action)
        return fail(CN_ERR_INVALID, "cn_step: action is required when robot_policy == CN_ROBOT_EXTERNAL");
    cn::StepIo io{action, reward, done, info, dmin, action_out, orca_vel, obs, update ? 1 : 0};
    pick_maxl_uni_kd(e, [&](auto maxl, auto uni, auto kd) {
        hipLaunchKernelGGL((cn::step_kernel<decltype(maxl)::value, decltype(uni)::value, decltype(kd)::value>), dim3(grid_envs(e)),
                           dim3(e->P.threads), e->smem, e->stream, e->P, e->S, io);
    });
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_set_gamma(cn_engine* e, double gamma) {
    int rc = bind(e);
    if (rc) return rc;
    const int len = (int)std::ceil(e->cfg.time_limit / e->cfg.time_step) + 8;
    if (len > cn::kMaxDiscount)
        return fail(CN_ERR_UNSUPPORTED, "time_limit / time_step = %d steps per episode exceeds the %d the rollout kernel tabulates",
                    len - 8, cn::kMaxDiscount - 8);
    std::vector<double> table((size_t)len);
    for (int t = 0; t < len; ++t) table[(size_t)t] = std::pow(gamma, t * e->cfg.time_step * e->cfg.robot_v_pref);
    CN_HIP(hipStreamSynchronize(e->stream));
    if (e->discount) CN_HIP(hipFree(e->discount));
    e->discount = nullptr;
    CN_HIP(hipMalloc(reinterpret_cast<void**>(&e->discount), sizeof(double) * len));
    CN_HIP(hipMemcpy(e->discount, table.data(), sizeof(double) * len, hipMemcpyHostToDevice));
    e->discount_len = len;
    return CN_OK;
}

// Upload the caller's io struct (ordered on the engine's stream) if it differs from the device copy.
static int upload_io(cn_engine* e, const cn_rollout_io* io) {
    if (e->io_valid && std::memcmp(&e->io_host, io, sizeof(*io)) == 0) return CN_OK;
    // the seed numbering belongs to cn_rollout_begin: the scenario cache was sized by seed_mod and filled for seed_base (a
    // larger seed_mod would index past it, another seed_base would be served the old seeds' scenarios)
    if (e->rollout_begun && (io->seed_base != e->begin_seed_base || io->seed_mod != e->begin_seed_mod))
        return fail(CN_ERR_INVALID, "rollout io: seed_base / seed_mod (%u / %u) differ from cn_rollout_begin's (%u / %u); call "
                    "cn_rollout_begin to renumber the episodes", io->seed_base, io->seed_mod, e->begin_seed_base, e->begin_seed_mod);
    int rc = e->ring.drain(e);
    if (rc) return rc;
    e->io_host = *io;
    CN_HIP(hipMemcpyAsync(e->io_dev, &e->io_host, sizeof(*io), hipMemcpyHostToDevice, e->stream));
    e->io_valid = true;
    return CN_OK;
}

static int check_io(const cn_engine* e, const cn_rollout_io* io) {
    if (!io) return fail(CN_ERR_INVALID, "rollout io is NULL");
    if (io->seed_mod == 0) return fail(CN_ERR_INVALID, "seed_mod must be >= 1");
    if (!io->ep_count || !io->cur_steps || !io->cur_return || !io->active)
        return fail(CN_ERR_INVALID, "rollout io: ep_count, cur_steps, cur_return and active are required");
    if (io->record_capacity < 0) return fail(CN_ERR_INVALID, "record_capacity must be >= 0");
    if (io->blocks && io->blocks_records < 1) return fail(CN_ERR_INVALID, "rollout io: blocks needs blocks_records >= 1");
    if (io->env_offset < 0 || io->env_stride < io->env_offset + e->P.B)
        return fail(CN_ERR_INVALID, "rollout io: need env_offset >= 0 and env_stride >= env_offset + num_envs");
    return CN_OK;
}

int cn_rollout_begin(cn_engine* e, const cn_rollout_io* io) {
    int rc = bind(e);
    if (rc) return rc;
    if ((rc = check_io(e, io)) || (rc = e->ring.drain(e))) return rc;
    e->rollout_begun = false;
    if ((rc = upload_io(e, io))) return rc;
    e->rollout_begun = true, e->begin_seed_base = io->seed_base, e->begin_seed_mod = io->seed_mod;
    if ((rc = e->ring.forget_first_steps(e))) return rc;
    return e->ring.begin(e, io->seed_mod);
}

// Which transition kernel a call runs: decided HERE, once (launch_rollout launches what this says; cn_rollout_route reports it).
// The four-barrier fused kernel (rollout_fused.h) takes the small-crowd geometries it covers, with BASELINE configs[1]'s
// geometry folded in as compile-time constants; that geometry's on-device rollout (no caller-supplied action) runs as the
// two-wave kernel when all its workgroups are resident at once; the 20-human shard has its own kernel; the general phase
// kernel takes everything else.
static int rollout_route(const cn_engine* e, const double* action) {
    const cn::Params& P = e->P;
    static const bool use_geom20 = env_int("CROWDNAV_AMD_GEOM20", 1) != 0;  // the compile-time geometry of configs[3]'s shard
    // (small crowds the fused kernel does not take — unicycle robot, asynchronous fill, several waves per workgroup — run the
    // generic rollout_kernel<5, ..>; its own compile-time-geometry instantiation for configs[1] went when the fused kernel
    // became the headline path)
    // (the fused kernel reads the launch-time fill level only: never with the asynchronous fill, whose slots are published
    // one by one — CROWDNAV_AMD_WAVE_SCENARIOS=1 can switch that on for a small crowd)
    if (e->use_fused && e->ring.mode != ScenarioRing::Fill::WorkList && e->maxl == 5 && !P.robot_unicycle && P.NC <= cn::kFusedMaxNC && P.pairs <= cn::kWave &&
        P.nA * 5 <= cn::kWave && P.threads == cn::kWave) {
#if defined(CN_PHASE_TIMING) || defined(CN_WAVE_TRACE)
        (void)action;
        return CN_ROUTE_FUSED;  // the probe builds instrument the one-wave kernel
#else
        const bool split = e->fused_split != 0 && headline_geometry(P) && P.robot_orca && action == nullptr &&
                           (grid_envs(e) <= e->split_slots || e->fused_split == 2);
        return split ? CN_ROUTE_FUSED_SPLIT : CN_ROUTE_FUSED;
#endif
    }
    if (use_geom20 && e->maxl == 10 && !P.robot_unicycle && P.A == 21 && P.NC == 20 && P.E == 1 && P.threads == 64 &&
        P.orca.max_neighbors == 10 && P.kd)
        return CN_ROUTE_SHARD;
    return CN_ROUTE_GENERIC;
}

// The 20-human shard's kernel (CN_ROUTE_SHARD) under one of its two schedules, or plain.
static void launch_shard(cn_engine* e, const cn::RolloutView& R, const int* levels, int n_steps, const double* action) {
    const cn::Params& P = e->P;
    const size_t smem20 = cn::smem_bytes_compact(P.nA, P.pairs, P.A, P.E);
    const auto launch = [&](const cn::Params& Pk, int grid, int steps) {
        hipLaunchKernelGGL((cn::rollout_kernel<10, false, true, true>), dim3(grid), dim3(64), smem20, e->stream, Pk,
                           (const cn::StateView*)e->S_dev, levels, R, steps, action);
    };
    // Three resident waves per SIMD (rollout_kernels.h: kGeom20Waves): 3072 one-wave workgroups fill the chip, so B = 4096 envs would run as
    // a full round plus a third of one.  A call of 3 q + r steps becomes one launch of r steps over all envs (if r > 0) and
    // FOUR launches of q steps over 3 B / 4 workgroups each, sub-launch k leaving out env 3 - k of every group of four
    // (step_kernels.h: Params::sched): every env makes its steps in order, every launch is one round.
    // Worth it when it saves rounds: with S = 12 workgroups x CUs resident, a plain launch takes ceil(B / S) rounds of
    // n steps, the schedule 4 ceil(0.75 B / S) rounds of n / 3 (B = 4096 on 256 CUs: 2 vs 1.33; B = 3072: 1 vs 1.33 - plain).
    // CROWDNAV_AMD_SCHED_MIN_STEPS / CROWDNAV_AMD_SCHED_FORCE (read_knobs): shortest call that is split; split
    // whatever the round count (the parity tests run the schedule on a handful of envs).
    cn::Params Pk = e->P;
    Pk.sched = -1;
    const int slots = e->sched_slots;
    // Dynamic schedule (rollout_kernels.h: kSchedDynamic): ONE launch of persistent workgroups taking (env, visit) items from a
    // device queue — wherever thirds of a call balance the chip better than whole calls (ceil(3 B / G) < 3 ceil(B / G)), and
    // always beside the asynchronous scenario fill, whose generator workgroups must find room WITHOUT sending a step workgroup
    // to a second round: the grid then leaves `sched_reserve` of the resident slots free (CROWDNAV_AMD_DYN_RESERVE).  Callers that
    // want the in-kernel summary / record blocks get the static 3-of-4 schedule below.
    const bool beside_generators = e->ring.mode == ScenarioRing::Fill::WorkList;
    const int reserve = beside_generators ? e->sched_reserve : 0;
    const int G = P.B < slots - reserve ? P.B : slots - reserve;
    // visits per env and call: ~56 steps each (measured at 4096 envs on the 12 m circle: 999-step calls 129 / 137 / 141 /
    // 143 / 143 / 136 / 110 M env-steps/s at 3 / 6 / 9 / 18 / 27 / 54 / 108 visits, 500-step calls 125 / 137 / 136 / 126 M
    // at 3 / 9 / 18 / 36 — shorter visits balance better until the per-visit prologue and the release / acquire of the
    // env's state show), at least three
    int visits = e->dyn_visits > 0 ? e->dyn_visits : (n_steps + 28) / 56;
    if (visits < 3) visits = 3;
    if (visits > n_steps) visits = n_steps;
    Pk.dyn_visits = visits;
    // work-conserving: worth it whenever the envs do not all fit at once (a plain launch then runs ceil(B / G) rounds)
    const bool helps = e->sched_force || beside_generators || P.B > G;
    if (e->sched_dynamic && G > 0 && n_steps >= e->sched_min && action == nullptr && helps && !e->io_host.summary &&
        !e->io_host.blocks) {
        (void)hipMemsetAsync(e->S.dyn_queue, 0, sizeof(int) * ((size_t)P.B + 1), e->stream);
        Pk.sched = cn::kSchedDynamic;
        e->launch_counts[CN_COUNT_ROLLOUT_KERNELS] += 1;
        e->launch_counts[CN_COUNT_SCHEDULED_KERNELS] += 1;
        launch(Pk, G, n_steps);
        return;
    }
    const int rounds_plain = (P.B + slots - 1) / slots, rounds_sched = (P.B / 4 * 3 + slots - 1) / slots;
    const bool sched = P.B % 4 == 0 && n_steps >= (e->sched_min > 48 ? e->sched_min : 48) && action == nullptr &&
                       (e->sched_force || 4 * rounds_sched < 3 * rounds_plain);
    const int q = sched ? n_steps / 3 : 0, rest = n_steps - 3 * q;
    e->launch_counts[CN_COUNT_ROLLOUT_KERNELS] += (rest > 0 ? 1 : 0) + (q > 0 ? 4 : 0);
    e->launch_counts[CN_COUNT_SCHEDULED_KERNELS] += q > 0 ? 4 : 0;
    if (rest > 0) launch(Pk, grid_envs(e), rest);
    for (int k = 0; k < 4 && q > 0; ++k) {
        Pk.sched = k;
        launch(Pk, P.B / 4 * 3, q);
    }
}

// n_steps >= 1 transitions of every env, by the kernel rollout_route names (R, levels: ScenarioRing::around_launch's)
static void launch_rollout(cn_engine* e, const cn::RolloutView& R, const int* levels, int n_steps, const double* action) {
    const int route = rollout_route(e, action);
    if (route == CN_ROUTE_SHARD) return launch_shard(e, R, levels, n_steps, action);  // (counts its own launches)
    if (route == CN_ROUTE_GENERIC)
        pick_maxl_uni_kd(e, [&](auto maxl, auto uni, auto kd) {
            hipLaunchKernelGGL((cn::rollout_kernel<decltype(maxl)::value, decltype(uni)::value, false, decltype(kd)::value>),
                               dim3(grid_envs(e)), dim3(e->P.threads), e->smem, e->stream, e->P, (const cn::StateView*)e->S_dev,
                               levels, R, n_steps, action);
        });
    else
        pick_fused(e, route, [&](auto kernel, int threads) {
            hipLaunchKernelGGL(kernel, dim3(grid_envs(e)), dim3(threads), e->smem, e->stream, e->P, (const cn::StateView*)e->S_dev,
                               levels, R, n_steps, action);
        });
    e->launch_counts[CN_COUNT_ROLLOUT_KERNELS] += 1;
}

// What cn_rollout, cn_rollout_trace, cn_rollout_step and cn_rollout_actions do before they launch: bind, check the io block and
// the call's length, upload the io block.  CN_OK: the entry point launches, through ScenarioRing::around_launch and in no other way.
// kNothingToLaunch: n_steps == 0.  kWrongRobotPolicy: the engine's robot policy is not the one the entry point is for;
// kNoAction: an external robot's entry point was given no action — no error text yet for these two, the entry point words it.
enum { kNothingToLaunch = 1, kWrongRobotPolicy = 2, kNoAction = 3 };
static int rollout_prepare(cn_engine* e, const cn_rollout_io* io, int n_steps, bool need_orca_robot,
                           const double* action = nullptr) {
    int rc = bind(e);
    if (rc) return rc;
    if ((rc = check_io(e, io))) return rc;
    if (n_steps < 0) return fail(CN_ERR_INVALID, "n_steps must be >= 0");
    if (n_steps == 0) return kNothingToLaunch;
    if ((e->P.robot_orca != 0) != need_orca_robot) return kWrongRobotPolicy;
    if (!need_orca_robot && !action) return kNoAction;
    return upload_io(e, io);
}

int cn_rollout(cn_engine* e, const cn_rollout_io* io, int n_steps) {
    const int rc = rollout_prepare(e, io, n_steps, true);
    if (rc == kNothingToLaunch) return CN_OK;
    if (rc == kWrongRobotPolicy)
        return fail(CN_ERR_UNSUPPORTED, "cn_rollout needs an on-device robot policy (robot_policy == CN_ROBOT_ORCA); with "
                                        "CN_ROBOT_EXTERNAL use cn_rollout_step(action)");
    if (rc) return rc;
    return e->ring.around_launch(e, n_steps, [&](const cn::RolloutView& R, const int* levels) {
        launch_rollout(e, R, levels, n_steps, nullptr);  // the fused transitions
    });
}

// cn_rollout with the per-step rows of `out`: cn_rollout's host path, then ONE launch of rollout_trace_kernel — the generic
// phase kernel's instantiation for the engine's half-plane capacity and kd bookkeeping — whatever the geometry.
int cn_rollout_trace(cn_engine* e, const cn_rollout_io* io, int n_steps, const cn_trace_out* out) {
    if (!e) return fail(CN_ERR_INVALID, "cn_rollout_trace: engine is NULL");
    if (!out) return fail(CN_ERR_INVALID, "cn_rollout_trace: out is NULL");
    if (!out->state8) return fail(CN_ERR_INVALID, "cn_rollout_trace: out->state8 is NULL");
    if (!out->episode) return fail(CN_ERR_INVALID, "cn_rollout_trace: out->episode is NULL");
    if (!out->step) return fail(CN_ERR_INVALID, "cn_rollout_trace: out->step is NULL");
    if (!e->P.robot_orca)
        return fail(CN_ERR_UNSUPPORTED, "cn_rollout_trace needs an on-device robot policy (robot_policy == CN_ROBOT_ORCA); with "
                                        "CN_ROBOT_EXTERNAL use cn_rollout_step(action)");
    const int rc = rollout_prepare(e, io, n_steps, true);
    if (rc == kNothingToLaunch) return CN_OK;
    if (rc) return rc;
    const cn_trace_out T = *out;
    return e->ring.around_launch(e, n_steps, [&](const cn::RolloutView& R, const int* levels) {
        pick_maxl(e, [&](auto maxl) {
            pick_bool(e->P.kd, [&](auto kd) {
                hipLaunchKernelGGL((cn::rollout_trace_kernel<decltype(maxl)::value, decltype(kd)::value>), dim3(grid_envs(e)),
                                   dim3(e->P.threads), e->smem, e->stream, e->P, (const cn::StateView*)e->S_dev, levels, R, n_steps,
                                   T);
            });
        });
        e->launch_counts[CN_COUNT_ROLLOUT_KERNELS] += 1;
    });
}

int cn_rollout_step(cn_engine* e, const cn_rollout_io* io, const double* action) {
    const int rc = rollout_prepare(e, io, 1, false, action);
    if (rc == kWrongRobotPolicy) return fail(CN_ERR_INVALID, "cn_rollout_step is for CN_ROBOT_EXTERNAL engines (use cn_rollout)");
    if (rc == kNoAction) return fail(CN_ERR_INVALID, "cn_rollout_step: action is NULL");
    if (rc) return rc;
    return e->ring.around_launch(e, 1, [&](const cn::RolloutView& R, const int* levels) { launch_rollout(e, R, levels, 1, action); });
}

// n_steps cn_rollout_step calls as one launch: cn_rollout's host path, then the generic phase kernel's table instantiation
// (rollout_actions_kernel, or rollout_actions_trace_kernel with the rows of `out`) whatever the geometry.  What depends on the
// arguments alone is refused first, then what depends on the engine; nothing is enqueued before the last check.
int cn_rollout_actions(cn_engine* e, const cn_rollout_io* io, int n_steps, const double* actions, const cn_trace_out* out) {
    if (!actions) return fail(CN_ERR_INVALID, "cn_rollout_actions: actions is NULL");
    if (out && !out->state8) return fail(CN_ERR_INVALID, "cn_rollout_actions: out->state8 is NULL");
    if (out && !out->episode) return fail(CN_ERR_INVALID, "cn_rollout_actions: out->episode is NULL");
    if (out && !out->step) return fail(CN_ERR_INVALID, "cn_rollout_actions: out->step is NULL");
    if (n_steps < 0) return fail(CN_ERR_INVALID, "n_steps must be >= 0");
    if (!e) return fail(CN_ERR_INVALID, "cn_rollout_actions: engine is NULL");
    if (e->P.robot_orca)
        return fail(CN_ERR_INVALID, "cn_rollout_actions is for CN_ROBOT_EXTERNAL engines (use cn_rollout)");
    const int rc = rollout_prepare(e, io, n_steps, false, actions);
    if (rc == kNothingToLaunch) return CN_OK;
    if (rc) return rc;
    return e->ring.around_launch(e, n_steps, [&](const cn::RolloutView& R, const int* levels) {
        pick_maxl_uni_kd(e, [&](auto maxl, auto uni, auto kd) {
            constexpr int kMaxl = decltype(maxl)::value;
            constexpr bool kUni = decltype(uni)::value, kKd = decltype(kd)::value;
            if (out)
                hipLaunchKernelGGL((cn::rollout_actions_trace_kernel<kMaxl, kUni, kKd>), dim3(grid_envs(e)), dim3(e->P.threads),
                                   e->smem, e->stream, e->P, (const cn::StateView*)e->S_dev, levels, R, n_steps, actions, *out);
            else
                hipLaunchKernelGGL((cn::rollout_actions_kernel<kMaxl, kUni, kKd>), dim3(grid_envs(e)), dim3(e->P.threads), e->smem,
                                   e->stream, e->P, (const cn::StateView*)e->S_dev, levels, R, n_steps, actions);
        });
        e->launch_counts[CN_COUNT_ROLLOUT_KERNELS] += 1;
    });
}

// K candidate sequences of n_steps actions per env, scored from the envs' current state in one launch of
// rollout_lookahead_kernel over B K virtual envs.  Not a rollout call: no io block, no ScenarioRing::around_launch (the ring is
// neither read nor filled, a pending lagged fill stays pending), no launch counter.  What depends on the arguments alone is
// refused first, then what depends on the engine; nothing is enqueued before the last check.  Under
// CN_HUMANS_CONSTANT_VELOCITY (cn_lookahead_set_human_model) the one launch is lookahead_cv_kernel's instead.
int cn_lookahead_actions(cn_engine* e, int n_steps, int n_candidates, const double* actions, const cn_lookahead_out* out) {
    int rc = cn_lookahead_check(e, n_steps, n_candidates, actions, out);
    if (rc || n_steps == 0) return rc;
    if ((rc = bind(e)) || (rc = upload_look(e, out))) return rc;
    const uint64_t virtual_envs = (uint64_t)e->P.B * (uint64_t)n_candidates;
    if (e->look_human_model == CN_HUMANS_CONSTANT_VELOCITY) {  // lookahead_cv_kernel.h: lane = branch, no ORCA
        const cn::CvParams C = cv_params(e, n_steps, n_candidates);
        // B * chunks <= B * K workgroups: within an int (cn_lookahead_check)
        pick_uni_goal(e, [&](auto uni, auto goal) {
            const dim3 grid((unsigned)C.B * (unsigned)C.chunks);
            if constexpr (decltype(goal)::value)
                hipLaunchKernelGGL((cn::lookahead_cv_goal_kernel<decltype(uni)::value>), grid, dim3(cn::kWave), 0, e->stream, C, actions,
                                   (const cn_lookahead_out*)e->look_dev, e->look_goal_weight);
            else
                hipLaunchKernelGGL((cn::lookahead_cv_kernel<decltype(uni)::value>), grid, dim3(cn::kWave), 0, e->stream, C, actions,
                                   (const cn_lookahead_out*)e->look_dev);
        });
        CN_HIP(hipGetLastError());
        return CN_OK;
    }
    if (look_goal(e) && (rc = upload_look_goal(e))) return rc;
    cn::Params Pv = e->P;
    Pv.B = (int)virtual_envs;
    const cn::RolloutView R{nullptr, e->discount, e->discount_len};
    pick_maxl_uni_kd(e, [&](auto maxl, auto uni, auto kd) {
        constexpr int kMaxl = decltype(maxl)::value;
        constexpr bool kUni = decltype(uni)::value, kKd = decltype(kd)::value;
        const dim3 grid((Pv.B + Pv.E - 1) / Pv.E);
        pick_bool(look_goal(e), [&](auto goal) {
            if constexpr (decltype(goal)::value)
                hipLaunchKernelGGL((cn::rollout_lookahead_goal_kernel<kMaxl, kUni, kKd>), grid, dim3(Pv.threads), e->smem, e->stream, Pv,
                                   (const cn::StateView*)e->S_dev, R, n_steps, actions, (const cn_lookahead_out*)e->look_dev,
                                   n_candidates);
            else
                hipLaunchKernelGGL((cn::rollout_lookahead_kernel<kMaxl, kUni, kKd>), grid, dim3(Pv.threads), e->smem, e->stream, Pv,
                                   (const cn::StateView*)e->S_dev, R, n_steps, actions, (const cn_lookahead_out*)e->look_dev,
                                   n_candidates);
        });
    });
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// The lookahead whose humans take the velocities the caller predicts: lookahead_paths_kernel (lookahead_cv_kernel.h), the
// constant-velocity kernel's lane body with human_vel[b][t][h] as the velocity a human chooses at step t.  cn_lookahead_actions' checks,
// upload and "nothing of the engine changes"; the engine's human-model setting is neither read nor written.
int cn_lookahead_paths(cn_engine* e, int n_steps, int n_candidates, const double* actions, const double* human_vel,
                       const cn_lookahead_out* out) {
    if (!human_vel) return fail(CN_ERR_INVALID, "cn_lookahead_paths: human_vel is NULL");
    int rc = cn_lookahead_check(e, n_steps, n_candidates, actions, out);
    if (rc || n_steps == 0) return rc;
    if ((rc = bind(e)) || (rc = upload_look(e, out))) return rc;
    const cn::CvParams C = cv_params(e, n_steps, n_candidates);
    pick_uni_goal(e, [&](auto uni, auto goal) {
        const dim3 grid((unsigned)C.B * (unsigned)C.chunks);
        if constexpr (decltype(goal)::value)
            hipLaunchKernelGGL((cn::lookahead_paths_goal_kernel<decltype(uni)::value>), grid, dim3(cn::kWave), 0, e->stream, C, actions,
                               human_vel, (const cn_lookahead_out*)e->look_dev, e->look_goal_weight);
        else
            hipLaunchKernelGGL((cn::lookahead_paths_kernel<decltype(uni)::value>), grid, dim3(cn::kWave), 0, e->stream, C, actions,
                               human_vel, (const cn_lookahead_out*)e->look_dev);
    });
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// cn_lookahead_paths against M tables at once, reduced per branch: lookahead_modes_kernel (lookahead_modes_kernel.h).  The
// refusals in the header's order; cn_lookahead_actions' own are made by cn_lookahead_check, which wants a cn_lookahead_out: the
// one handed to it names out->score in every required place and is only tested for NULL.  `modes` and `out` travel as kernel
// arguments, so no device copy of either is kept and nothing of the engine is written.
int cn_lookahead_modes(cn_engine* e, int n_steps, int n_candidates, const double* actions, const cn_path_modes* modes,
                       const cn_modes_out* out) {
    if (!modes) return fail(CN_ERR_INVALID, "cn_lookahead_modes: modes is NULL");
    if (!modes->human_vel) return fail(CN_ERR_INVALID, "cn_lookahead_modes: modes->human_vel is NULL");
    if (!out) return fail(CN_ERR_INVALID, "cn_lookahead_modes: out is NULL");
    if (!out->score) return fail(CN_ERR_INVALID, "cn_lookahead_modes: out->score is NULL");
    if (modes->n_modes < 1) return fail(CN_ERR_INVALID, "cn_lookahead_modes: n_modes must be >= 1 (got %d)", modes->n_modes);
    if (modes->n_modes > cn::kModesMax)
        return fail(CN_ERR_UNSUPPORTED, "cn_lookahead_modes: n_modes = %d exceeds the %d modes a lane keeps in registers",
                    modes->n_modes, cn::kModesMax);
    if (modes->reduce != CN_MODES_MEAN && modes->reduce != CN_MODES_MIN)
        return fail(CN_ERR_INVALID, "cn_lookahead_modes: reduce %d unknown (CN_MODES_MEAN = 0, CN_MODES_MIN = 1)", modes->reduce);
    if (!(modes->risk_penalty >= 0.0) || !std::isfinite(modes->risk_penalty))
        return fail(CN_ERR_INVALID, "cn_lookahead_modes: risk_penalty must be >= 0 and finite (got %g)", modes->risk_penalty);
    const cn_lookahead_out probe{out->score, reinterpret_cast<uint8_t*>(out->score), reinterpret_cast<int32_t*>(out->score),
                                 out->score, nullptr, nullptr};
    int rc = cn_lookahead_check(e, n_steps, n_candidates, actions, &probe);
    if (rc) return rc;
    const uint64_t mode_rows = (uint64_t)e->P.B * (uint64_t)n_candidates * (uint64_t)modes->n_modes;
    if (mode_rows > (uint64_t)INT32_MAX)
        return fail(CN_ERR_UNSUPPORTED, "cn_lookahead_modes: num_envs * n_candidates * n_modes = %llu exceeds the %llu per-mode "
                    "rows a launch indexes", (unsigned long long)mode_rows, (unsigned long long)INT32_MAX);
    if (n_steps == 0) return CN_OK;
    if ((rc = bind(e))) return rc;
    const cn::CvParams C = cv_params(e, n_steps, n_candidates);
    const cn::ModesParams Q{modes->n_modes, modes->reduce, modes->risk_penalty, modes->human_vel, modes->weight, *out};
    const size_t lds = cn::modes_lds_bytes(Q.M, C.A - 1);  // at most 4 * 504 * 16 + 63 * 8 = 32760 bytes
    pick_uni_goal(e, [&](auto uni, auto goal) {
        const dim3 grid((unsigned)C.B * (unsigned)C.chunks);
        if constexpr (decltype(goal)::value)
            hipLaunchKernelGGL((cn::lookahead_modes_goal_kernel<decltype(uni)::value>), grid, dim3(cn::kWave), lds, e->stream, C, actions,
                               Q, e->look_goal_weight);
        else
            hipLaunchKernelGGL((cn::lookahead_modes_kernel<decltype(uni)::value>), grid, dim3(cn::kWave), lds, e->stream, C, actions, Q);
    });
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// how the humans of a lookahead's branches move: a host-side setting of the engine, nothing of the device is touched
int cn_lookahead_set_human_model(cn_engine* e, int model) {
    if (!e) return fail(CN_ERR_INVALID, "cn_lookahead_set_human_model: engine is NULL");
    if (model != CN_HUMANS_ORCA && model != CN_HUMANS_CONSTANT_VELOCITY)
        return fail(CN_ERR_INVALID, "cn_lookahead_set_human_model: model %d unknown (CN_HUMANS_ORCA = 0, "
                    "CN_HUMANS_CONSTANT_VELOCITY = 1)", model);
    e->look_human_model = model;
    return CN_OK;
}

int cn_lookahead_get_human_model(const cn_engine* e, int* model_host) {
    if (!e) return fail(CN_ERR_INVALID, "cn_lookahead_get_human_model: engine is NULL");
    if (!model_host) return fail(CN_ERR_INVALID, "cn_lookahead_get_human_model: model_host is NULL");
    *model_host = e->look_human_model;
    return CN_OK;
}

// the goal-progress term of every lookahead's return: a host-side setting of the engine, nothing of the device is touched.
// What depends on the argument alone is refused first.  -0.0 is not negative (IEEE: -0.0 < 0.0 is false): it is accepted and
// means 0.0, the plain kernels.
int cn_lookahead_set_goal_weight(cn_engine* e, double weight) {
    if (!std::isfinite(weight) || weight < 0.0)
        return fail(CN_ERR_INVALID, "cn_lookahead_set_goal_weight: weight must be >= 0 and finite (got %g)", weight);
    if (!e) return fail(CN_ERR_INVALID, "cn_lookahead_set_goal_weight: engine is NULL");
    e->look_goal_weight = weight;
    return CN_OK;
}

int cn_lookahead_get_goal_weight(const cn_engine* e, double* weight_host) {
    if (!e) return fail(CN_ERR_INVALID, "cn_lookahead_get_goal_weight: engine is NULL");
    if (!weight_host) return fail(CN_ERR_INVALID, "cn_lookahead_get_goal_weight: weight_host is NULL");
    *weight_host = e->look_goal_weight;
    return CN_OK;
}

int cn_rollout_route(cn_engine* e, int n_steps, int* route_host) {
    if (!e || !route_host) return fail(CN_ERR_INVALID, "cn_rollout_route: NULL argument");
    if (n_steps < 0) return fail(CN_ERR_INVALID, "n_steps must be >= 0");
    *route_host = rollout_route(e, nullptr);  // (no route depends on the call's length today; the shard's schedules are not routes)
    return CN_OK;
}

int cn_lagged_fills(cn_engine* e, uint64_t* count_host) {
    if (!e || !count_host) return fail(CN_ERR_INVALID, "cn_lagged_fills: NULL argument");
    *count_host = e->ring.lagged_fills;
    return CN_OK;
}

int cn_fresh_starts(cn_engine* e, uint64_t* counts_host) {
    int rc = bind(e);
    if (rc) return rc;
    if (!counts_host) return fail(CN_ERR_INVALID, "cn_fresh_starts: counts_host is NULL");
    unsigned int dev[2] = {0u, 0u};
    CN_HIP(hipMemcpyAsync(dev, e->S.fresh_counts, sizeof(dev), hipMemcpyDeviceToHost, e->stream));
    CN_HIP(hipStreamSynchronize(e->stream));
    counts_host[0] = dev[0], counts_host[1] = dev[1], counts_host[2] = e->ring.first_step_kernels;
    return CN_OK;
}

int cn_ring_slot(cn_engine* e, int env, int slot, double* state8_host, float* vel0_host, int* ok_host) {
    int rc = bind(e);
    if (rc || (rc = e->ring.settle(e))) return rc;
    if (!state8_host || !vel0_host || !ok_host) return fail(CN_ERR_INVALID, "cn_ring_slot: NULL argument");
    if (env < 0 || env >= e->P.B || slot < 0 || slot >= e->P.ring_mod)
        return fail(CN_ERR_INVALID, "cn_ring_slot: (env, slot) = (%d, %d) outside %d envs x %d slots", env, slot, e->P.B, e->P.ring_mod);
    const int A = e->P.A;
    const size_t idx = (size_t)env * e->P.ring_mod + slot;
    std::vector<double2> pos((size_t)A), goal((size_t)A), rv((size_t)A);
    std::vector<float2> vel((size_t)A, make_float2(0.0f, 0.0f));
    uint8_t ok = 0;
    CN_HIP(hipStreamSynchronize(e->stream));
    CN_HIP(hipMemcpy(pos.data(), e->S.ring_pos + idx * A, sizeof(double2) * A, hipMemcpyDeviceToHost));
    CN_HIP(hipMemcpy(goal.data(), e->S.ring_goal + idx * A, sizeof(double2) * A, hipMemcpyDeviceToHost));
    CN_HIP(hipMemcpy(rv.data(), e->S.ring_rv + idx * A, sizeof(double2) * A, hipMemcpyDeviceToHost));
    if (e->ring.first_step) {
        CN_HIP(hipMemcpy(vel.data(), e->S.ring_vel0 + idx * A, sizeof(float2) * A, hipMemcpyDeviceToHost));
        CN_HIP(hipMemcpy(&ok, e->S.ring_vel0_ok + idx, 1, hipMemcpyDeviceToHost));
    }
    for (int a = 0; a < A; ++a) {
        double* s = state8_host + 8 * (size_t)a;
        s[0] = pos[a].x, s[1] = pos[a].y, s[2] = 0.0, s[3] = 0.0, s[4] = goal[a].x, s[5] = goal[a].y, s[6] = rv[a].x, s[7] = rv[a].y;
        vel0_host[2 * a] = vel[a].x, vel0_host[2 * a + 1] = vel[a].y;
    }
    *ok_host = ok;
    return CN_OK;
}

int cn_launch_counts(cn_engine* e, uint64_t* counts_host) {
    if (!e || !counts_host) return fail(CN_ERR_INVALID, "cn_launch_counts: NULL argument");
    for (int i = 0; i < CN_LAUNCH_COUNTERS; ++i) counts_host[i] = e->launch_counts[i];
    return CN_OK;
}

int cn_rollout_records(cn_engine* e, const cn_rollout_io* io, int max_records, double* blocks) {
    int rc = bind(e);
    if (rc) return rc;
    if ((rc = check_io(e, io))) return rc;
    if (max_records < 1 || !blocks) return fail(CN_ERR_INVALID, "cn_rollout_records: need max_records >= 1 and blocks");
    if ((rc = upload_io(e, io))) return rc;
    const int n = e->P.B * max_records;
    hipLaunchKernelGGL(cn::records_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->P.B, max_records, e->io_dev,
                       blocks);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_records_summary(cn_engine* e, int64_t n_envs, int max_records, int record_capacity, const double* blocks,
                       double* summary) {
    int rc = bind(e);
    if (rc) return rc;
    if (n_envs < 0 || max_records < 1 || record_capacity < 0 || !blocks || !summary)
        return fail(CN_ERR_INVALID, "cn_records_summary: bad arguments");
    const cn::BlockRecords src{blocks, cn::record_block_doubles(max_records)};
    if (n_envs * max_records <= cn::kSummarySmallItems)
        hipLaunchKernelGGL(cn::records_summary_small_kernel<cn::BlockRecords>, dim3(1), dim3(cn::kSummarySmallThreads), 0, e->stream,
                           n_envs, max_records, record_capacity, src, summary);
    else
        hipLaunchKernelGGL(cn::records_summary_kernel<cn::BlockRecords>, dim3(cn::kSummaryBlocks), dim3(cn::kSummaryThreads), 0,
                           e->stream, n_envs, max_records, record_capacity, src, summary, e->summary_scratch);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

int cn_rollout_summary(cn_engine* e, const cn_rollout_io* io, double* summary) {
    int rc = bind(e);
    if (rc) return rc;
    if ((rc = check_io(e, io))) return rc;
    if (!summary) return fail(CN_ERR_INVALID, "cn_rollout_summary: summary is NULL");
    if (io->record_capacity < 1) return fail(CN_ERR_INVALID, "cn_rollout_summary: the rollout keeps no records (record_capacity 0)");
    if ((rc = upload_io(e, io))) return rc;
    if ((int64_t)e->P.B * io->record_capacity <= cn::kSummarySmallItems)
        hipLaunchKernelGGL(cn::records_summary_small_kernel<cn::RingRecords>, dim3(1), dim3(cn::kSummarySmallThreads), 0, e->stream,
                           (int64_t)e->P.B, io->record_capacity, io->record_capacity, cn::RingRecords{e->io_dev}, summary);
    else
        hipLaunchKernelGGL(cn::records_summary_kernel<cn::RingRecords>, dim3(cn::kSummaryBlocks), dim3(cn::kSummaryThreads), 0,
                           e->stream, (int64_t)e->P.B, io->record_capacity, io->record_capacity, cn::RingRecords{e->io_dev}, summary,
                           e->summary_scratch);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

// RCCL is bound at first use (dlopen of librccl.so.1: in a PyTorch-ROCm process that is the copy torch already loaded),
// so the library itself does not depend on it.
namespace {
struct RcclApi {
    int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t);
    const char* (*error_string)(int);
    bool ok;
};
const RcclApi* rccl_api() {
    static RcclApi api = [] {
        RcclApi a{};
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return a;
        a.all_gather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(h, "ncclAllGather"));
        a.error_string = reinterpret_cast<const char* (*)(int)>(dlsym(h, "ncclGetErrorString"));
        a.ok = a.all_gather && a.error_string;
        return a;
    }();
    return &api;
}
constexpr int kNcclFloat64 = 8;  // ncclDataType_t (rccl.h)
}  // namespace

int cn_gather_records(cn_engine* e, void* rccl_comm, int n_ranks, int max_records, const double* blocks,
                      double* blocks_all) {
    int rc = bind(e);
    if (rc) return rc;
    if (!rccl_comm || n_ranks < 1 || max_records < 1 || !blocks || !blocks_all)
        return fail(CN_ERR_INVALID, "cn_gather_records: bad arguments");
    const RcclApi* api = rccl_api();
    if (!api->ok) return fail(CN_ERR_UNSUPPORTED, "cn_gather_records: librccl.so.1 could not be loaded");
    const size_t n = (size_t)e->P.B * cn::record_block_doubles(max_records);
    const int st = api->all_gather(blocks, blocks_all, n, kNcclFloat64, rccl_comm, e->stream);
    if (st) return fail(CN_ERR_HIP, "cn_gather_records: RCCL error %d (%s)", st, api->error_string(st));
    return CN_OK;
}

int cn_mt_random(cn_engine* e, uint32_t seed, int n, double* out) {
    int rc = bind(e);
    if (rc) return rc;
    if (n < 0 || !out) return fail(CN_ERR_INVALID, "cn_mt_random: bad arguments");
    hipLaunchKernelGGL(cn::mt_probe_kernel, dim3(1), dim3(1), 0, e->stream, e->probe_key, seed, n, out);
    CN_HIP(hipGetLastError());
    return CN_OK;
}

}  // extern "C"

// Which workgroup geometry pick_geometry gave this engine after its clamps: envs per workgroup, threads per workgroup, LDS bytes
// per workgroup and the grid of the per-env kernels.  For the tests that ask for a geometry through the tuning knobs; host-only,
// not part of the public header.
extern "C" int cn_debug_geometry(const cn_engine* e, int out[4]) {
    if (!e || !out) return fail(CN_ERR_INVALID, "cn_debug_geometry: NULL argument");
    out[0] = e->P.E;
    out[1] = e->P.threads;
    out[2] = (int)e->smem;
    out[3] = grid_envs(e);
    return CN_OK;
}

#ifdef CN_PHASE_TIMING
// profiling builds only (scripts/phase_probe.py): accumulated shader-clock cycles per rollout phase, [8] = waves
extern "C" int cn_debug_phase_cycles(unsigned long long* out16, int reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(cn::cn_phase_cycles), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[16] = {};
        zero[13] = ~0ull;  // the fastest wave's total (atomicMin)
        if (hipMemcpyToSymbol(HIP_SYMBOL(cn::cn_phase_cycles), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef CN_PHASE_TIMING
extern "C" int cn_debug_lazy_counts(unsigned long long* out8, int reset) {
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(cn::cn_lazy_counts), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(cn::cn_lazy_counts), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef CN_SPLIT_PROBE
extern "C" int cn_debug_split_probe(unsigned long long* out32, int reset) {
    if (out32 && hipMemcpyFromSymbol(out32, HIP_SYMBOL(cn::cn_split_probe), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[32] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(cn::cn_split_probe), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef CN_WAVE_TRACE
extern "C" int cn_debug_wave_trace(unsigned long long* out, int waves) {
    if (waves > 8192) waves = 8192;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(cn::cn_wave_trace), (size_t)waves * 6 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
