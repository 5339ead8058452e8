/*
 * crowdnav_amd.h — C ABI of libcrowdnav_amd.so, the MI355X (gfx950) batched crowd-navigation engine.
 *
 * The reference (vita-epfl/CrowdNav) has NO C ABI for this path: its boundary is the Python plugin API
 *   crowd_sim/envs/crowd_sim.py:51-79,251-420   CrowdSim.configure / reset / step / onestep_lookahead
 *   crowd_sim/envs/policy/orca.py:82-132        ORCA.predict  (-> rvo2.PyRVOSimulator, the only native code)
 *   crowd_nav/utils/explorer.py:21-90           Explorer.run_k_episodes
 * Each entry point below names the reference interface it replaces.  The Python host side
 * (crowdnav_amd/) binds these with ctypes and mirrors the reference's classes on top; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (CN_OK) or a negative cn_status; cn_last_error() gives the message of the
 *     last failure on the calling thread; nothing throws across the ABI.
 *   - all data pointers are DEVICE pointers (hipMalloc'd, e.g. a torch tensor's data_ptr()) unless the
 *     parameter name ends in _host.  The caller owns them and keeps them alive until the stream is synced.
 *   - calls are asynchronous on the engine's stream (cn_set_stream; default = the null stream) unless
 *     documented otherwise.  An engine is bound to one device and is not thread-safe.
 *   - agent 0 of every env is the robot, agents 1..H are the humans; A = H + 1.
 *   - batched state layout ("state8"): double [B][A][8] = px, py, vx, vy, gx, gy, radius, v_pref
 *     (crowd_sim/envs/utils/state.py:1-50 minus theta: the robot's heading is a separate [B] plane,
 *     cn_set_theta / cn_get_theta; only a unicycle robot changes it).
 */
#ifndef CROWDNAV_AMD_H
#define CROWDNAV_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cn_status {
    CN_OK = 0,
    CN_ERR_INVALID = -1,     /* bad argument / config            */
    CN_ERR_UNSUPPORTED = -2, /* valid in the reference, not built here (e.g. a value network under the mixed rule) */
    CN_ERR_HIP = -3,         /* a HIP runtime call failed         */
    CN_ERR_NO_DEVICE = -4    /* no gfx950 device visible          */
} cn_status;

/* info codes returned by step (crowd_sim/envs/utils/info.py:1-38) */
enum { CN_NOTHING = 0, CN_DANGER = 1, CN_REACH_GOAL = 2, CN_COLLISION = 3, CN_TIMEOUT = 4 };
/* robot_policy */
enum { CN_ROBOT_EXTERNAL = 0, CN_ROBOT_ORCA = 1 };
/* robot_kinematics */
enum { CN_HOLONOMIC = 0, CN_UNICYCLE = 1 };
/* scenario_rule (crowd_sim.py:84-153) */
enum { CN_CIRCLE_CROSSING = 0, CN_SQUARE_CROSSING = 1, CN_MIXED = 2 };

/* Everything CrowdSim.configure (crowd_sim.py:51-79), the [humans]/[robot] sections read by Agent.__init__
 * (crowd_sim/envs/utils/agent.py:10-31) and the hard-coded ORCA parameters (orca.py:60-66) provide. */
typedef struct cn_config {
    int32_t num_envs;   /* B */
    int32_t num_humans; /* H, 1..63 */
    double time_step;
    double time_limit;
    double success_reward;
    double collision_penalty;
    double discomfort_dist;
    double discomfort_penalty_factor;
    int32_t robot_visible; /* humans' ORCA sees the robot (crowd_sim.py:326-327) */
    int32_t robot_policy;  /* CN_ROBOT_EXTERNAL: caller supplies the action; CN_ROBOT_ORCA: solved on device */
    double robot_safety_space;
    double human_safety_space;
    double neighbor_dist;  /* 10 */
    int32_t max_neighbors; /* 10 (<= 10 supported) */
    int32_t scenario_rule;
    double time_horizon;      /* 5 */
    double time_horizon_obst; /* 5, unused: the reference never adds obstacles */
    double circle_radius;
    double square_width;
    double human_radius;
    double human_v_pref;
    double robot_radius;
    double robot_v_pref;
    int32_t randomize_attributes; /* agent.py:39-45 */
    int32_t device;               /* HIP device ordinal */
    int32_t robot_kinematics;     /* CN_HOLONOMIC: actions are ActionXY(vx, vy); CN_UNICYCLE: ActionRot(v, r)
                                     (agent.py:115-135; CN_ROBOT_EXTERNAL only - the ORCA policy is holonomic) */
    int32_t flags;                /* CN_FLAG_* */
} cn_config;

/* cn_config.flags */
/* Generate the scenarios of cn_rollout / cn_rollout_step's auto-resets ASYNCHRONOUSLY: the fill kernels run on the engine's
 * own side streams next to the transition kernels and publish every scenario on its own (per-slot ready flag, release /
 * acquire at device scope), so a launch never waits for the hardest scenario of the batch — only the env whose NEXT
 * scenario is not ready yet pauses (it steps again in a later launch).  Trajectories and episode records are unchanged;
 * how many transitions a launch executes becomes timing-dependent.  For crowds whose rejection sampling
 * (crowd_sim.py:155-176) is heavy-tailed: 20 humans on the 4 m circle need 28 k random() calls per scenario on average and
 * 10+ M for the worst.  More than 8 humans only (the wave-cooperative generators). */
#define CN_FLAG_ASYNC_SCENARIO_FILL 1

typedef struct cn_engine cn_engine;

/* message of the last failed call on this thread ("" if none) */
const char* cn_last_error(void);
/* ABI version of this header (bumped on any change of a signature or of what a call does).  v10 (round 6): no new symbol —
 * cn_sarl_sample_step skips the envs outside `alive` on its two-launch route, takes CN_MODEL_LSTM_RL there and accepts `info` in
 * pinned host memory; cn_rollout / cn_rollout_step / the boundary calls refuse an io whose seed_base / seed_mod differ from
 * cn_rollout_begin's.  v11 (round 6): + cn_sarl_values.  v12: + cn_sarl_select_attention. */
#define CN_ABI_VERSION 12
int cn_abi_version(void);

/* replaces gym.make('CrowdSim-v0') + CrowdSim.configure + set_robot (crowd_sim.py:13-82): allocates the
 * SoA state of B envs in HBM.  Synchronous. */
int cn_create(const cn_config* cfg, cn_engine** out);
int cn_destroy(cn_engine* e);
/* hipStream_t the engine launches on (pass torch.cuda.current_stream().cuda_stream); NULL = null stream */
int cn_set_stream(cn_engine* e, void* hip_stream);
/* blocks until everything queued on the engine's stream is done */
int cn_sync(cn_engine* e);

/* teacher forcing / inspection: copy state8 [B][A][8] f64 and global_time [B] f64 (either may be NULL).
 * replaces Agent.set / get_full_state (agent.py:47-108). */
int cn_set_state(cn_engine* e, const double* state8, const double* global_time);
int cn_get_state(cn_engine* e, double* state8, double* global_time);
/* robot heading theta, double [B] (FullState.theta; reset sets pi/2, crowd_sim.py:274; only a unicycle robot changes it) */
int cn_set_theta(cn_engine* e, const double* theta);
int cn_get_theta(cn_engine* e, double* theta);
/* len(env.humans) of every env, int32 [B].  Only the `mixed` rule (crowd_sim.py:103-151) draws the number of humans
 * per episode (0..5 static obstacles — 0 leaves the reference's single placeholder human at (0, -10) — or 1..5 moving
 * humans: two circle-crossing, the rest square-crossing).  The engine keeps num_humans slots per env; absent humans are
 * parked at rest at x >= 1e6, out of every neighbour range, and sit AFTER the present ones in cn_get_state / obs. */
int cn_get_human_count(cn_engine* e, int32_t* count);
/* forget the robot ORCA policy's captured radii and its rvo2 simulator's kd-tree order (a new policy object;
 * orca.py:95-104) */
int cn_drop_robot_sim(cn_engine* e);
/* (ABI v5) forget EVERY agent's rvo2 simulator — the robot's as above and each human's (a human's ORCA policy object and
 * its simulator are rebuilt with the Human at every CrowdSim.reset, crowd_sim.py:155-207; cn_reset and the rollout's
 * auto-reset do this themselves).  What a simulator carries from step to step besides the radii is the permutation its
 * kd-tree partitions in place (RVO2 KdTree::buildAgentTree; only simulators of more than 10 agents ever split): it decides
 * the visiting order of candidates at EXACTLY equal squared distance.  For a caller that teleports the agents with
 * cn_set_state and wants the behaviour of freshly built simulators. */
int cn_drop_sims(cn_engine* e);
/* The opposite: give every env the SAME captured simulator — radii host float32 [num_humans + 1] (robot, humans) as
 * the robot's rvo2 simulator holds them (radius + 0.01 + safety_space), max_speed its maxSpeed.  This is what one
 * persistent ORCA policy object means for a batch: the reference builds the simulator at the policy's first predict and
 * keeps those radii for every later episode (orca.py:95-110), so k episodes run as a batch must all see the radii of
 * the policy's first episode (only observable with randomize_attributes). */
int cn_set_robot_sim(cn_engine* e, const float* radii_host, float max_speed);

/* replaces CrowdSim.reset (crowd_sim.py:251-312) for the envs with mask[b] != 0 (mask NULL = all):
 * np.random.seed(seeds[b]) + generate_random_human_position, numpy-MT19937-compatible, on device.
 * draws (optional, uint64 [B]) receives the number of np.random.random() calls consumed. */
int cn_reset(cn_engine* e, const uint32_t* seeds, const uint8_t* mask, uint64_t* draws);

/* replaces Human.act/Robot.act -> ORCA.predict -> rvo2 doStep -> getAgentVelocity(0) for EVERY agent of
 * every env from the current state (orca.py:82-132): out_vel float [B][A][2].  Agent 0 is solved with the
 * robot's ORCA parameters whatever robot_policy is. */
int cn_orca(cn_engine* e, float* out_vel);

/* replaces CrowdSim.step(action, update) / onestep_lookahead (crowd_sim.py:314-420).
 *   action      double [B][2] (ActionXY vx, vy - or ActionRot v, r for a CN_UNICYCLE robot), NULL iff robot_policy ==
 *               CN_ROBOT_ORCA
 *   reward      double [B]; done uint8 [B]; info uint8 [B] (CN_*); dmin double [B] (+inf if no human checked)
 *   action_out  double [B][2] action actually applied (optional)
 *   orca_vel    float [B][A][2] velocity chosen by every agent (optional)
 *   obs         double [B][H][5] humans' ObservableState px,py,vx,vy,radius AFTER the step (update=1) or
 *               their next observable state (update=0, agent.py:63-74) (optional) */
int cn_step(cn_engine* e, const double* action, int update, double* reward, uint8_t* done, uint8_t* info,
            double* dmin, double* action_out, float* orca_vel, double* obs);

/* Episode bookkeeping of Explorer.run_k_episodes (explorer.py:35-72), kept per env on device. */
typedef struct cn_rollout_io {
    /* episode numbering: local env b has global env id g = env_offset + b and runs the global episode ids
     * c = g + j*env_stride (j = 0,1,..) while c < episode_limit; episode c is seeded
     * np.random.seed(seed_base + c % seed_mod) (crowd_sim.py:272-283).  A single engine uses env_offset 0,
     * env_stride B; rank r of W uses env_offset r*B, env_stride W*B, so the set of episodes and every
     * trajectory is independent of how the env axis is sharded. */
    uint32_t seed_base;
    uint32_t seed_mod;
    int64_t episode_limit; /* <0: unbounded */
    int64_t env_offset;
    int64_t env_stride;    /* >= env_offset + B */
    int32_t record_capacity; /* records kept per env: a RING — episode j of the env lands in slot j % record_capacity, so
                                once an env has finished more than record_capacity episodes slot j holds its most recent
                                episode with ordinal congruent to j (older ones are overwritten) */
    /* per-episode records, [B][record_capacity]; all optional */
    uint8_t* ep_outcome;   /* CN_REACH_GOAL / CN_COLLISION / CN_TIMEOUT */
    int32_t* ep_steps;
    double* ep_return;     /* sum_t gamma^(t*dt*v_pref) * r_t, python left-to-right order (explorer.py:71-72) */
    double* ep_time;       /* env.global_time at the end (explorer.py:52-62) */
    int32_t* ep_danger;    /* number of Danger steps (explorer.py:46-48) */
    double* ep_danger_dmin_sum;
    /* per-env counters, [B], in/out; the caller zeroes them before the first launch */
    int32_t* ep_count;     /* episodes finished so far by env b */
    int32_t* cur_steps;    /* steps into the running episode */
    double* cur_return;
    int32_t* cur_danger;
    double* cur_danger_dmin_sum;
    uint8_t* active;       /* 0 once env b ran out of episodes (c >= episode_limit) */
    uint64_t* transitions; /* [1] device counter: += number of step() transitions executed */
    /* (ABI v5) shard-boundary outputs produced by the LAST workgroup of every cn_rollout / cn_rollout_step launch itself
     * (arrival tickets, fixed summation order: bitwise reproducible), so that a single-GPU run needs no boundary kernel
     * and a sharded run only its all-gather.  Both optional (NULL = off): */
    double* summary;       /* [CN_SUMMARY_FIELDS] the numbers of cn_records_summary over THIS engine's record rings */
    double* blocks;        /* [B][CN_RECORD_BLOCK_DOUBLES(blocks_records)] what cn_rollout_records(blocks_records) packs */
    int32_t blocks_records; /* >= 1 when blocks != NULL */
    /* (ABI v6) per-env transition counters, [B], optional: env b's entry grows by the transitions env b made in the call.
     * With `transitions` and `summary` both NULL a launch ends WITHOUT any hand-off between workgroups (no arrival tickets: ~9 us
     * of the last wave's tail): whoever wants a job-wide number sums this array, and computes the statistics once per run with
     * cn_rollout_records + cn_records_summary — which is when explorer.py:74-90 computes them. */
    uint64_t* env_transitions;
} cn_rollout_io;

/* discount table used for ep_return: gamma^(t * time_step * robot_v_pref), computed on the host with libm
 * pow exactly as explorer.py:71 does.  Synchronous. */
int cn_set_gamma(cn_engine* e, double gamma);

/* (re)start episode bookkeeping: every env b with b < episode_limit is reset to its episode j=0 scenario
 * and the per-env counters of io are zeroed.  Crowds of more than 8 humans (the wave-cooperative generators): when io.seed_mod <=
 * 4096 — the episode seeds come from a small set, as in the reference's 'val' / 'test' phases (crowd_sim.py:272-283) — the rollout
 * keeps every scenario it has generated and copies it when the same seed comes round again (a seeded scenario is a pure function
 * of its seed; CROWDNAV_AMD_SCENARIO_CACHE=0 switches this off).  Same scenarios, same episodes. */
int cn_rollout_begin(cn_engine* e, const cn_rollout_io* io);
/* replaces the `while not done: action = robot.act(ob); env.step(action)` loop of
 * Explorer.run_k_episodes (explorer.py:41-48) for an on-device robot policy (robot_policy ==
 * CN_ROBOT_ORCA): n_steps transitions per active env in ONE call, with in-kernel auto-reset.  A call is one kernel launch
 * over all envs, except on the 20-human shard geometry (20 humans + robot, max_neighbors 10, holonomic), whose kernel keeps S =
 * 12 x CUs one-wave workgroups resident: when B > S (or beside the asynchronous scenario fill, or with
 * CROWDNAV_AMD_SCHED_FORCE=1) a call of n >= 24 steps (CROWDNAV_AMD_SCHED_MIN_STEPS; the static form: 48) runs under a SCHEDULE:
 *   - dynamic (default): ONE launch of min(B, S) persistent workgroups that take (env, visit) items from a device queue — a call
 *     is max(3, n / 56) visits per env (CROWDNAV_AMD_DYN_VISITS), an env's visits in order (release / acquire on a per-env word):
 *     the chip stays full whatever B / S is, and nothing waits at a launch boundary for the slowest wave of a round;
 *   - static (CROWDNAV_AMD_SCHED_DYNAMIC=0, and whenever io.summary or io.blocks is set; needs B % 4 == 0 and
 *     4 ceil(0.75 B / S) < 3 ceil(B / S)): one launch of n % 3 steps over all envs and four launches of n / 3 steps over three
 *     envs of every four (the in-kernel statistics cover every env: the last sub-launch reports for the env it leaves out).
 * Every env makes its n transitions in order either way: per-env state, per-env counters and episode records are bit-identical
 * to an unscheduled call; the float64 SUMS of io.summary (nav time, return) are accumulated in a different workgroup order under
 * the static schedule and may differ from an unscheduled call's, and from cn_records_summary's, in the last bits (counts are
 * exact).  cn_launch_counts reports what a call launched. */
int cn_rollout(cn_engine* e, const cn_rollout_io* io, int n_steps);

/* (ABI v7) what the HOST has enqueued for this engine since cn_create — counts_host: HOST uint64 [CN_LAUNCH_COUNTERS], indexed
 * by CN_COUNT_*; synchronous, no device work.  Lets a caller (bench.py, the parity tests) state which launches a timed region
 * contained — e.g. whether a cn_rollout call carried a scenario fill (the ring budget rule: a fill only when the steps since the
 * last one exceed the ring depth) and whether the 20-human shard's 3-of-4 env schedule was taken — instead of inferring it. */
enum {
    CN_COUNT_ROLLOUT_KERNELS = 0,   /* transition kernels launched by cn_rollout / cn_rollout_step */
    CN_COUNT_SCHEDULED_KERNELS = 1, /* ... of which launches of the shard kernel's schedules: one per call under the dynamic
                                       schedule, four per call (sub-launches) under the static 3-of-4 one */
    CN_COUNT_RING_FILLS = 2,        /* scenario-ring fills of the lane-per-scenario and the synchronous wave generators: one per
                                       cn_rollout call that carried one, in front of its launch or (lagged fill) beside it */
    CN_COUNT_ASYNC_FILLS = 3,       /* fill launches on the side streams (CN_FLAG_ASYNC_SCENARIO_FILL: one per call) */
    CN_COUNT_SARL_NARROW = 4,       /* (ABI v9) value-network launches on the narrow tiles (cn_sarl_select / cn_sarl_sample_step
                                       of a few envs): which route a decision took */
    CN_COUNT_SARL_DECIDE_STEPS = 5  /* (ABI v9) cn_sarl_sample_step calls that ran decision + transition + next ORCA as ONE kernel */
};
#define CN_LAUNCH_COUNTERS 6
int cn_launch_counts(cn_engine* e, uint64_t* counts_host);

/* (no ABI bump: a new symbol only) how many of the CN_COUNT_RING_FILLS fills were LAGGED — count_host: HOST uint64.  Engines of
 * at most 8 humans without CN_FLAG_ASYNC_SCENARIO_FILL keep 2 D ring slots per env (D = CROWDNAV_AMD_RING_DEPTH, default 48) and
 * top the ring up on a side stream beside a launch, for the call after it, whenever a repeat of the current call would need a
 * fill; a launch still sees at most D scenarios ahead of each env, so results are those of the synchronous fill.
 * CROWDNAV_AMD_LAGGED_FILL=0 (read by cn_create) keeps D slots and fills in front of the launch only. */
int cn_lagged_fills(cn_engine* e, uint64_t* count_host);

/* (no ABI bump: new symbols only) Engines whose cn_rollout runs the two-wave kernel (CN_ROUTE_FUSED_SPLIT) solve the first ORCA
 * step of every ring scenario when its slot is filled; an episode that starts inside a launch then adopts those velocities and
 * the workgroup does not compute that step a second time.  Results are bit-identical either way.
 * cn_fresh_starts — counts_host: HOST uint64 [3], since cn_create: [0] episode starts that adopted solved velocities, [1]
 * iterations a workgroup computed again because an episode start could not (slot unsolved, env paused or retired), [2] launches
 * of the solving kernel.  Waits for the engine's stream.
 * cn_ring_slot — ring slot `slot` (0 .. slots per env - 1; ordinal o lives in slot o % slots) of env `env` as the last fill left
 * it: state8_host HOST double [A][8] (get_state's layout, velocities 0), vel0_host HOST float [A][2] and *ok_host (1: vel0_host
 * is the slot's solved first step; always 0 on other engines).  Waits for the fills that are out and the engine's stream. */
int cn_fresh_starts(cn_engine* e, uint64_t* counts_host);
int cn_ring_slot(cn_engine* e, int env, int slot, double* state8_host, float* vel0_host, int* ok_host);

/* (no ABI bump: a new symbol only) which transition kernel cn_rollout(e, io, n_steps) would launch NOW — route_host: HOST int,
 * one of CN_ROUTE_*.  Host-only: launches nothing, counts nothing.  The fused two-wave kernel (rollout_fused.h) takes the
 * headline geometry — 5 humans + ORCA robot, 2 envs per workgroup — when every workgroup of the launch is resident at once
 * (workgroups <= CUs x the occupancy the runtime reports for the kernel) and CROWDNAV_AMD_FUSED_SPLIT is not 0 (read by
 * cn_create, like CROWDNAV_AMD_FUSED; 2 takes it for launches of several rounds as well — slower there, for measurements); its
 * results are bit-identical to the one-wave kernel's. */
enum {
    CN_ROUTE_GENERIC = 0,     /* rollout_kernel, the phase kernel */
    CN_ROUTE_FUSED = 1,       /* rollout_fused_kernel, one wave per workgroup */
    CN_ROUTE_FUSED_SPLIT = 2, /* rollout_fused_kernel, an ORCA wave and an env wave per workgroup */
    CN_ROUTE_SHARD = 3        /* the 20-human shard's kernel, under a schedule or not */
};
int cn_rollout_route(cn_engine* e, int n_steps, int* route_host);

/* ------------------------------------------------------------------------------------------------------
 * SARL robot decision (crowd_nav/policy/sarl.py:9-86 on top of multi_human_rl.py:11-63, cadrl.py:82-222).
 * Needs robot_policy == CN_ROBOT_EXTERNAL: the chosen action is then applied with cn_step(action). */
/* value network behind cn_sarl_select:
 *   CN_MODEL_SARL   sarl.ValueNetwork (attention over humans, sarl.py:9-65).  Every model takes any num_humans the engine
 *                   holds (<= 63): crowds beyond one tile's LDS (6+ humans at the shipped SARL widths, 9+ for CADRL /
 *                   LSTM-RL) stream through the tile in chunks; occupancy maps and LSTM-RL's distance ordering likewise.
 *   CN_MODEL_CADRL  cadrl.ValueNetwork: one MLP per (robot, human) pair, value = min over humans
 *                   (crowd_nav/policy/cadrl.py:22-29, 156-168); only mlp3_dims (= [cadrl] mlp_dims), n_actions, gamma
 *                   are read; cn_sarl_set_weights then takes 8 pointers (value_network.{0,2,4,6}.{weight,bias})
 *   CN_MODEL_LSTM_RL lstm_rl.ValueNetwork1 (LSTM over the humans + value head, lstm_rl.py:9-33; the variant the shipped
 *                   policy.config selects, with_interaction_module = false): mlp1_dims[0] = [lstm_rl] global_state_dim,
 *                   mlp3_dims = [lstm_rl] mlp2_dims, with_om as configured; cn_sarl_set_weights takes 12 pointers
 *                   (mlp.{0,2,4,6}.{weight,bias}, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0).
 *                   interaction_dims[0] > 0 selects lstm_rl.ValueNetwork2 (with_interaction_module = true,
 *                   lstm_rl.py:36-66): every human's input row first passes mlp1 = [lstm_rl] mlp1_dims (4 layers, ReLU
 *                   between them) and the LSTM runs over mlp1's outputs; cn_sarl_set_weights then takes 20 pointers:
 *                   mlp1.{0,2,4,6}.{weight,bias} followed by the 12 above (the module's state_dict order) */
enum { CN_MODEL_SARL = 0, CN_MODEL_CADRL = 1, CN_MODEL_LSTM_RL = 2 };

typedef struct cn_sarl_config {
    int32_t n_actions;          /* 81 = speed_samples * rotation_samples + 1 (cadrl.py:82-102) */
    int32_t with_om;            /* [sarl] with_om: append the occupancy map (multi_human_rl.py:109-163) */
    int32_t cell_num;           /* [om] cell_num */
    int32_t om_channel_size;    /* [om] om_channel_size: 1, 2 or 3 */
    double cell_size;           /* [om] cell_size */
    double gamma;               /* [rl] gamma */
    int32_t with_global_state;  /* [sarl] with_global_state */
    int32_t mlp1_dims[2];       /* [sarl] mlp1_dims      (150, 100) */
    int32_t mlp2_dims[2];       /* [sarl] mlp2_dims      (100, 50) */
    int32_t attention_dims[3];  /* [sarl] attention_dims (100, 100, 1) */
    int32_t mlp3_dims[4];       /* [sarl] mlp3_dims      (150, 100, 100, 1); CN_MODEL_CADRL: [cadrl] mlp_dims */
    int32_t model;              /* CN_MODEL_SARL (0), CN_MODEL_CADRL (1) or CN_MODEL_LSTM_RL (2) */
    int32_t interaction_dims[4];/* CN_MODEL_LSTM_RL only: [lstm_rl] mlp1_dims (150, 100, 100, 50) when
                                   with_interaction_module, else all 0 */
    int32_t constant_velocity_model; /* 0: [action_space] query_env = true — next human states and reward from the env's
                                   onestep_lookahead (multi_human_rl.py:37-38).  1: query_env = false — every human keeps
                                   its observed velocity for one step and the reward is MultiHumanRL.compute_reward
                                   (multi_human_rl.py:39-42, 65-88: end-point distances, constants -0.25 / 1 / 0.2 / 0.5, no
                                   time limit); for CN_MODEL_LSTM_RL the humans then enter the network in the order
                                   LstmRL.predict sorted them (decreasing distance to the robot, lstm_rl.py:96-103).
                                   SARL / LSTM-RL only: CADRL.predict always queries the env. */
    int32_t precision;          /* (the former `reserved` word: no ABI bump, zero keeps every caller's meaning) CN_PRECISION_*:
                                   the arithmetic of the value network's linear layers in cn_sarl_select /
                                   cn_sarl_select_attention / cn_sarl_sample_step at the sizes that leave the narrow tiles.
                                   CN_PRECISION_F32 (0): fp32 matrix instructions, as ever.  CN_PRECISION_F16X2 (1): the
                                   split-f16 route — every weight and every activation as two f16 terms (x ~ xh + xl / 2^11),
                                   three f16 matrix products per layer in two fp32 accumulators, everything between the
                                   layers in fp32: values within 1e-6 of the fp32 routes on the shipped networks (DESIGN.md
                                   §3.9).  CN_MODEL_SARL at the shipped layer widths (13- or 61-wide rows, with_global_state
                                   = 1) and 1..5 humans, not under the `mixed` rule; cn_sarl_configure returns
                                   CN_ERR_UNSUPPORTED with the reason for anything else (it never falls back) and
                                   CN_ERR_INVALID for any other value of this word.  An activation beyond the f16 range
                                   (|a| > 65504; the shipped networks stay below 100) makes that env's values NaN, hence
                                   best = -2: never a wrong finite value.  The narrow tiles (a few envs) and cn_sarl_values
                                   stay fp32. */
} cn_sarl_config;
enum { CN_PRECISION_F32 = 0, CN_PRECISION_F16X2 = 1 };

/* replaces SARL.configure + CADRL.build_action_space: actions_host = double [n_actions][2] (ActionXY table, HOST
 * pointer, computed by the caller exactly as cadrl.py:86-99 does).  Synchronous; once per engine.
 * Layer widths are free (the shipped ones have register-resident kernels).  A sarl.ValueNetwork whose tile — one (env, action)
 * group's activations for all humans plus the pipelined side buffer, 4 x 64 x (H (ks_a + ks_b + ks_c + 4) + ks_b + 3 ks_a) bytes,
 * ks = the widest layer of each buffer in 4-column steps — exceeds the 160 KiB of LDS streams the humans through in chunks
 * instead (at 5 humans: a first mlp1 / mlp3 layer wider than 160); under the `mixed` rule, whose one-tile kernel masks absent
 * humans, such a network is CN_ERR_UNSUPPORTED.
 * What "free" ends at, each CN_ERR_UNSUPPORTED with its reason (tests/test_net_widths.py): a layer of more than 1020 inputs or
 * 4080 outputs (the packed descriptors hold 255 k-steps and 255 column tiles); a network beyond the 16 MiB weight arena; a
 * network whose STREAMED form — five humans at a time, 4 x (64 x (5 (ks_a + ks_b + ks_c + 4) + ks_b + 2 ks_a + ks_c + 1) + 1024)
 * bytes — exceeds the 160 KiB as well (mlp1 272,100 in front of the shipped layers does: 202 496 B); CN_MODEL_CADRL, which
 * streams only beyond 8 humans, when 4 x 64 x H (ks_a + ks_b + 4) does (mlp_dims 272,100,36,1 at 8 humans). */
int cn_sarl_configure(cn_engine* e, const cn_sarl_config* cfg, const double* actions_host);
/* replaces model.load_state_dict: params_host_array = HOST array of 22 DEVICE pointers to the float32 tensors of
 * sarl.ValueNetwork.state_dict() in its own order (mlp1.0.weight, mlp1.0.bias, mlp1.2.*, mlp2.0.*, mlp2.2.*,
 * attention.0.*, attention.2.*, attention.4.*, mlp3.0.*, mlp3.2.*, mlp3.4.*, mlp3.6.*); weights are [out][in]
 * row-major as torch stores them.  Repacked into MFMA operand order on device; call again after every optimizer
 * step whose result the rollout should see. */
int cn_sarl_set_weights(cn_engine* e, const float* const* params_host_array);
/* replaces the greedy branch of MultiHumanRL.predict (multi_human_rl.py:32-58) for every env:
 *   values  double [B][n_actions] (optional) reward(lookahead) + gamma^(dt*v_pref) * V(next state)
 *   best    int32  [B] index of the first strict maximum; -1 = robot already at its goal -> stop action (:22-23);
 *                  -2 = no finite value (the reference raises ValueError, :57-58)
 *   action  double [B][2] the chosen ActionXY */
int cn_sarl_select(cn_engine* e, double* values, int32_t* best, double* action);
/* (ABI v12) cn_sarl_select plus the attention weights of every (env, action) group — what sarl.ValueNetwork.forward keeps
 * of batch element 0 (sarl.py:52-54) and SARL.get_attention_weights returns (sarl.py:88-89), for every lookahead state:
 *   attention  float32 [B][n_actions][num_humans]: exp(s_h) [s_h != 0] / sum over the humans present, humans in env order
 *              as the network saw them; 0 for the absent humans of a `mixed` episode; a group whose scores are all exactly
 *              zero gets the kernel's 0 / 0 (NaN), as the reference does.
 * The weights are a by-product of the decision's own network kernel (no second pass): values / best / action are
 * bit-identical to cn_sarl_select's on the same state, and attention == NULL IS cn_sarl_select.  CN_MODEL_SARL only:
 * CN_MODEL_CADRL and CN_MODEL_LSTM_RL (no attention in the reference) return CN_ERR_UNSUPPORTED. */
int cn_sarl_select_attention(cn_engine* e, double* values, int32_t* best, double* action, float* attention);
/* (no ABI bump: a new symbol only) which kernel family runs the value network of this configuration — route_host: HOST int,
 * one of CN_SARL_ROUTE_*, chosen once by cn_sarl_configure.  Host-only: launches nothing, counts nothing. */
enum {
    CN_SARL_ROUTE_LDS_TILE = 0,       /* a tile's activations in LDS, a workgroup per tile */
    CN_SARL_ROUTE_LDS_CHUNKED = 1,    /* ... the humans streamed through the tile in chunks */
    CN_SARL_ROUTE_NARROW = 2,         /* a few decisions on 16-row tiles */
    CN_SARL_ROUTE_REG_SARL = 3,       /* activations in registers, a wave per tile: sarl.ValueNetwork, 1..5 humans */
    CN_SARL_ROUTE_REG_SARL_CHUNK = 4, /* ... 6+ humans */
    CN_SARL_ROUTE_REG_CADRL = 5,
    CN_SARL_ROUTE_REG_LSTM = 6,
    CN_SARL_ROUTE_REG_LSTM2 = 7,
    CN_SARL_ROUTE_SPLIT_F16 = 8       /* CN_PRECISION_F16X2: activations in registers, split-f16 matrix instructions */
};
int cn_sarl_network_route(cn_engine* e, int* route_host);
/* replaces the epsilon-greedy branch of MultiHumanRL.predict in the train phase (multi_human_rl.py:28-31), applied to
 * the best/action a cn_sarl_select just produced: per env (mask == NULL or mask[b] != 0, and not already at its goal)
 *   probability = np.random.random(); if probability < epsilon: action_space[np.random.choice(n_actions)]
 * drawn from the env's OWN numpy stream — the one cn_reset seeded (np.random.seed, crowd_sim.py:272-276) continued
 * after the scenario draws, exactly as the sequential reference consumes it.  Needs episodes started by cn_reset
 * (otherwise the next cn_sync fails); both scenario generators (one lane / one wave per scenario) leave the env's
 * generator where the scenario's last draw left it.  explored (optional) uint8 [B]: 1 where the random action was taken. */
int cn_sarl_explore(cn_engine* e, double epsilon, const uint8_t* mask, int32_t* best, double* action,
                    uint8_t* explored);
/* replaces MultiHumanRL.transform (multi_human_rl.py:90-104; CADRL.transform cadrl.py:171-185 for one human) for the
 * CURRENT joint state of every env — the state a train-phase predict() leaves in policy.last_state and
 * Explorer.update_memory (explorer.py:92-125) pushes into the replay memory:
 *   out float32, env b's [H][13 (+ cell_num^2 * om_channel_size)] block at out + b * env_stride (floats;
 *   0 = densely packed [B][H][D]; a larger stride writes step t of a [B][T][H][D] trajectory tensor in place).
 * sort_humans != 0 (meaningful for CN_MODEL_LSTM_RL): the humans appear by decreasing distance to the robot, as
 * LstmRL.predict re-orders them before it stores last_state (lstm_rl.py:96-103; stable for equal distances) — the RL
 * phase; 0 = env order, which is what imitation learning stores (explorer.py:99 transforms the ORCA robot's own state). */
int cn_sarl_transform(cn_engine* e, float* out, int64_t env_stride, int sort_humans);
/* (ABI v8) replaces ONE iteration of the train-phase sampling loop, Explorer.run_k_episodes' `while not done: action =
 * robot.act(ob); ob, reward, done, info = env.step(action)` (explorer.py:56-65) with MultiHumanRL.predict behind robot.act
 * (multi_human_rl.py:11-63) — for every env, in this order and with these results:
 *   alive[b] &= !done[b]                              (the previous call's episode ends: an env samples until its episode is over;
 *                                                      the caller zeroes done before an episode's first call)
 *   cn_sarl_select(e, NULL, best, action)
 *   cn_sarl_explore(e, epsilon, alive, best, action, NULL)
 *   cn_sarl_transform(e, state_out, env_stride, sort_humans)      (state_out == NULL: skipped)
 *   cn_step(e, action, 1, reward, done, info, dmin, NULL, NULL, NULL)
 * as one call.  For a FEW envs (CN_MODEL_SARL with or without occupancy maps, or CN_MODEL_CADRL; up to 8 humans, at most one
 * workgroup per CU: 9 envs of 5 humans x 81 actions — BASELINE configs[4]'s one episode at a time, train.py:156-170) a streamed
 * loop of these calls is TWO launches per step instead of eight: the value network on tiles of 16 / num_humans whole
 * (env, action) groups, one per workgroup — a decision spread over 27 CUs instead of 6, its input rows built in LDS, each
 * tile adding the lookahead reward of its own groups and writing env b's replay-memory state on an idle wave; then ONE kernel
 * for the arg-max, the epsilon-greedy draw, the transition and the humans' ORCA velocities (with occupancy maps also their next
 * states and the maps) of the NEXT decision.  Those
 * velocities are trusted by the next call only if no other entry point of this engine ran in between (any of them may change
 * the state they belong to); otherwise, and on the first call, ORCA is a launch of its own in front.  Same bits as the five
 * calls above in every case (tests/test_rl_pipeline.py).  cn_sarl_select takes the same network kernel at these sizes (two
 * launches less).  CROWDNAV_AMD_SARL_NARROW=0 keeps the one-tile kernels, 2 takes the narrow tiles at any size the
 * configuration allows; CROWDNAV_AMD_SARL_FUSED_STEP=0 (and workgroups of several waves / simulators of more than 10
 * agents): ORCA, the network with the decision by its last workgroup, the transition — three launches.
 * Round 6: CN_MODEL_LSTM_RL (lstm_rl.ValueNetwork1, the environment queried) takes the two launches as well; the transition
 * kernel reuses the humans' ORCA velocities the decision's lookahead was given (one ORCA pass per step); and on the two-launch
 * route an env OUTSIDE alive (its episode is over) is SKIPPED: no decision, no replay-memory state, no transition — its
 * state, its done flag and its entries of reward / info / dmin / best / state_out stay as its last sampled step left them
 * (the other routes keep stepping such an env, as cn_step does; either way those outputs mean nothing).  A caller that
 * cannot know an episode's end without a round trip may therefore stream a few calls past it at the price of two
 * near-empty launches each; info — and reward / dmin / best, which that route only writes, a step's before its info code and
 * an episode's last step's acknowledged before it — (written, never read, by the kernels) may point into pinned host memory so that the host
 * sees the episode-end codes arrive without synchronising (compat.Explorer._run_batched_rl). */
int cn_sarl_sample_step(cn_engine* e, double epsilon, uint8_t* alive, int32_t* best, double* action, float* state_out,
                        int64_t env_stride, int sort_humans, double* reward, uint8_t* done, uint8_t* info, double* dmin);
/* (ABI v11) V(state) of n joint states the CALLER holds — float32 [n][num_humans][13] rows in the layout cn_sarl_transform /
 * cn_sarl_sample_step write (a replay memory's states) — under the weights last given to cn_sarl_set_weights: what
 * `target_model(next_states)` is to the TD targets of Explorer.update_memory (crowd_nav/utils/explorer.py:113-116), on the
 * narrow tiles (sarl_narrow_kernel: ONE launch, the rows read where they lie) instead of the ~35 library kernels of a
 * framework forward on a few dozen rows.  out: float32 [n].  The env state of the engine is neither read nor written — an engine
 * that only serves a target network needs no reset.  CN_MODEL_SARL / CN_MODEL_LSTM_RL (ValueNetwork1) without occupancy maps
 * at a size that takes the narrow tiles (cn_sarl_sample_step's conditions), 1 <= n <= num_envs x n_actions; CN_ERR_UNSUPPORTED
 * otherwise.  Same arithmetic as the decision's network kernel (tests/test_sarl.py: <= 2e-6 of the framework's forward). */
int cn_sarl_values(cn_engine* e, const float* states, int64_t n, float* out);
/* test/inspection: copy an internal buffer of the last cn_sarl_select to dst (device pointer):
 *   0 reward f64 [B][K] · 1 V f32 [B*K] · 2 next human states f64 [B][H][5] · 3 occupancy maps f32 [B][H][cells*ch]
 *   4 X f32 in MLP tile order (see sarl_kernels.h) */
int cn_sarl_export(cn_engine* e, int which, void* dst, uint64_t bytes);

/* The same episode loop for a robot whose policy lives OUTSIDE the engine (robot_policy == CN_ROBOT_EXTERNAL, e.g. the
 * SARL decision of cn_sarl_select): ONE transition of every running env with action double [B][2], plus all of
 * cn_rollout's bookkeeping and seeded auto-reset from the scenario ring — `action = robot.act(ob); env.step(action)`
 * of explorer.py:41-48 without leaving the device. */
int cn_rollout_step(cn_engine* e, const cn_rollout_io* io, const double* action);

/* ------------------------------------------------------------------------------------------------------
 * Shard boundary: the statistics block of Explorer.run_k_episodes (explorer.py:50-62, 71-90) needs every finished
 * episode on one rank.  The env axis is sharded over GPUs with NO collective on the step path (cn_rollout_io.env_offset /
 * env_stride); the only exchange is one all-gather of fixed-size per-env record blocks when a run ends. */
#define CN_RECORD_FIELDS 6  /* outcome (CN_*), steps, discounted return, nav time, danger steps, danger dmin sum */
#define CN_SUMMARY_FIELDS 8
/* doubles per env in a record block holding up to K records: { episodes finished, K x CN_RECORD_FIELDS } */
#define CN_RECORD_BLOCK_DOUBLES(K) (1 + (K) * CN_RECORD_FIELDS)
/* pack the record rings of io into ONE self-contained float64 block per env: blocks double
 * [B][CN_RECORD_BLOCK_DOUBLES(max_records)]; block b = { number of episodes env b has finished (unclamped), then record j
 * = ring slot j for j < min(count, record_capacity, max_records), zeros beyond }.  Slot j is the env's j-th finished episode
 * while count <= record_capacity; after the ring has wrapped it is the most recent episode with ordinal = j mod
 * record_capacity (size the rings for the episodes a run can finish when per-episode identities matter).  One kernel. */
int cn_rollout_records(cn_engine* e, const cn_rollout_io* io, int max_records, double* blocks);
/* all-gather such blocks over the ranks of an RCCL communicator (rccl_comm = the caller's ncclComm_t, one rank per GPU;
 * librccl.so.1 is bound at first use): blocks_all double [n_ranks * B][CN_RECORD_BLOCK_DOUBLES(max_records)], rank-major
 * = ordered by global env id, identical on every rank.  ONE ncclAllGather on the engine's stream (200 KiB per rank at
 * 4096 envs, max_records 1: latency-bound).  A reference process that owns one engine per GPU calls this where
 * explorer.py:74 starts. */
int cn_gather_records(cn_engine* e, void* rccl_comm, int n_ranks, int max_records, const double* blocks,
                      double* blocks_all);
/* explorer.py:74-90 on record blocks (a shard's own or the gathered ones): summary double [CN_SUMMARY_FIELDS] =
 * episodes finished, records held, ReachGoal / Collision / Timeout among them, sum of the successful nav times, sum of
 * the discounted returns, sum of the Danger steps.  record_capacity = the capacity of the rings the blocks were packed
 * from (records beyond it are not counted).  One kernel, fixed summation order (bitwise reproducible; rates and averages
 * are quotients of these). */
int cn_records_summary(cn_engine* e, int64_t n_envs, int max_records, int record_capacity, const double* blocks,
                       double* summary);
/* (ABI v6) the same numbers for THIS engine's own record rings, without packing blocks first: what a single-engine run calls
 * where explorer.py:74 starts (bitwise equal to cn_records_summary over cn_rollout_records(record_capacity)). */
int cn_rollout_summary(cn_engine* e, const cn_rollout_io* io, double* summary);

/* numpy legacy RNG probe (np.random.seed(seed); n × np.random.random()): out double [n].  For tests. */
int cn_mt_random(cn_engine* e, uint32_t seed, int n, double* out);

/* ------------------------------------------------------------------------------------------------------
 * Device SGD step (added after v12, no version bump: purely additive).  Replaces ONE iteration of Trainer.optimize_epoch /
 * optimize_batch (crowd_nav/utils/trainer.py:21-23, 56-66):
 *   optimizer.zero_grad(); loss = MSELoss()(model(x), y); loss.backward(); optimizer.step()
 * with optim.SGD(lr, momentum) — dampening 0, no weight decay, no Nesterov — for crowd_nav/policy/sarl.py:9-65 or
 * crowd_nav/policy/lstm_rl.py:9-33 as two launches, float32 throughout.  A trainer needs no environments and is therefore not a cn_engine; it keeps NO copy of the
 * parameters: they and their momentum buffers are the caller's tensors, updated in place, so state_dict(), checkpoints,
 * update_target_model and cn_sarl_set_weights see them as after a framework step.
 * Built for two networks, the shipped widths only; anything else is CN_ERR_UNSUPPORTED with a message that names the field and
 * the value (n_actions, gamma, cell_size and the other fields of net are not read):
 *   CN_MODEL_SARL     with_global_state = 1, mlp1 150,100 / mlp2 100,50 / attention 100,100,1 / mlp3 150,100,100,1: 22 tensors.
 *   CN_MODEL_LSTM_RL  lstm_rl.ValueNetwork1 under the convention of cn_sarl_config above: mlp1_dims = (hidden, 1) with hidden =
 *                     50, mlp3_dims = the value head 150,100,100,1 (its input: 6 self-state columns + hidden), interaction_dims
 *                     all zero (non-zero = lstm_rl.ValueNetwork2: refused): 12 tensors.  The humans are the LSTM's steps in the
 *                     order of the rows; torch's gate order i, f, g, o.
 * Both: input width 13 + (with_om ? cell_num^2 * om_channel_size : 0) <= 64, 1..8 humans, batches of 1..128.
 * cn_trainer_create validates and touches no device; the first cn_train_step probes it and allocates the scratch rows
 * (make that call outside a stream capture; every later one is two kernel launches and capturable). */
typedef struct cn_trainer cn_trainer;
int cn_trainer_create(const cn_sarl_config* net, int num_humans, int max_batch, int device, cn_trainer** out);
int cn_trainer_destroy(cn_trainer* t);
int cn_trainer_set_stream(cn_trainer* t, void* hip_stream);
/* params_host_array / momentum_host_array: HOST arrays of 22 (CN_MODEL_SARL) or 12 (CN_MODEL_LSTM_RL: mlp.{0,2,4,6}.{weight,
 * bias}, lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) DEVICE pointers in state_dict order (as cn_sarl_set_weights
 * takes them), every one non-NULL, weights [out][in] row-major; a zero momentum buffer gives the framework's first step (buf = g).
 * states float32 [rows][num_humans][D] and values float32 [rows] are read WHERE THEY LIE — a replay ring — through
 * index int64 [n] (device; NULL = rows 0..n-1); an index outside [0, rows) is clamped into it rather than read out of bounds.
 * Per parameter tensor: buf = momentum_factor * buf + g; p -= lr * buf, g summed over the batch rows in row order by one
 * owner per entry (no atomics: the same inputs give the same bits).  loss_sum (optional, device, float64): the batch's MSE
 * is ADDED to it.  Asynchronous on the trainer's stream. */
int cn_train_step(cn_trainer* t, float* const* params_host_array, float* const* momentum_host_array, const float* states,
                  const float* values, int64_t rows, const int64_t* index, int64_t n, double lr, double momentum_factor,
                  double* loss_sum);
/* steps_host (HOST pointer): cn_train_step calls of this trainer that launched their kernels. */
int cn_trainer_steps(const cn_trainer* t, int64_t* steps_host);

/* ------------------------------------------------------------------------------------------------------
 * Per-step record of a batched ORCA rollout (added after v12, no version bump: purely additive).  The reference keeps
 * env.states for every episode it runs (crowd_sim/envs/crowd_sim.py:246,393: the joint state is appended BEFORE the step);
 * cn_rollout returns per-episode totals only.  cn_rollout_trace(e, io, n, out) changes the engine and io exactly as
 * cn_rollout(e, io, n) does — same checks, same scenario-ring fill, same states, counters, records, transitions, summary /
 * blocks; the two may be mixed freely on one rollout — and writes row [b][t] of `out` for the t-th step of THIS call:
 *   - an env that makes a transition at step t: every non-NULL array's row;
 *   - an env that is retired (episode_limit reached) or waiting for a scenario: episode[b][t] = -1, nothing else;
 *   - the state AFTER an episode's last transition is not recorded: the next row is the next episode's reset state, step 0;
 *   - humans absent under the `mixed` rule show as the parked placeholders cn_get_state shows.
 * Always ONE launch of the generic phase kernel (counted under CN_COUNT_ROLLOUT_KERNELS, never under
 * CN_COUNT_SCHEDULED_KERNELS): the fused small-crowd kernel and the 20-human shard kernel are not involved, so a traced call
 * is slower than cn_rollout — this is the inspection path.  64 A + 8 bytes per env-step, 17 more with all optional arrays.
 * NULL e / out / state8 / episode / step: CN_ERR_INVALID; CN_ROBOT_EXTERNAL: CN_ERR_UNSUPPORTED (use cn_rollout_step).
 * Asynchronous on the engine's stream. */
typedef struct cn_trace_out {      /* all DEVICE pointers */
    double*  state8;   /* [B][n_steps][A][8]  required: the state before the transition, as cn_get_state lays it out */
    int32_t* episode;  /* [B][n_steps]        required: ordinal j of the env's episode (global id env_offset + b + j * env_stride); -1 = no transition */
    int32_t* step;     /* [B][n_steps]        required: index of the transition inside its episode (0 = from the reset state) */
    double*  reward;   /* [B][n_steps]        optional (NULL = off): what cn_step returns for that transition */
    uint8_t* info;     /* [B][n_steps]        optional: CN_NOTHING .. CN_TIMEOUT */
    double*  dmin;     /* [B][n_steps]        optional */
} cn_trace_out;
int cn_rollout_trace(cn_engine* e, const cn_rollout_io* io, int n_steps, const cn_trace_out* out);

/* ------------------------------------------------------------------------------------------------------
 * Open-loop action table (added after v12, no version bump: purely additive).  Replaces the `while not done: action =
 * robot.act(ob); env.step(action)` loop of Explorer.run_k_episodes (explorer.py:41-48) for a robot whose actions are KNOWN IN
 * ADVANCE — a planner scoring candidate action sequences, the recorded actions of an evaluation replayed for its states, the
 * reference's own episodes re-run: cn_rollout_actions(e, io, n, actions, out) does exactly what n consecutive
 * cn_rollout_step(e, io, a_t) calls do, with a_t[b] = actions[b][t], in ONE call and one launch — the same transitions,
 * bookkeeping, seeded auto-reset from the scenario ring, per-env counters, records, transitions / env_transitions, summary /
 * blocks, the same checks and scenario-ring fill as cn_rollout(e, io, n); it may be mixed freely with cn_rollout_step on one
 * rollout.
 *   - actions: DEVICE double [B][n_steps][2].  Row t belongs to step t of THIS call, not to a step index inside an episode;
 *     an env that is retired or waiting for a scenario at step t ignores its row t.  Holonomic engines read a row as (vx, vy),
 *     CN_UNICYCLE engines as (v, r): the heading is carried across the steps and is pi / 2 at every episode start.
 *   - as in cn_rollout, an env that finishes more episodes inside one call than the ring holds ahead of it pauses until the
 *     next call.
 *   - out (optional, NULL = no per-step rows): the rows of cn_rollout_trace, by its rules — state8, episode and step required,
 *     reward, info and dmin optional, arrays [B][n_steps], episode pre-filled with -1 by the caller.
 * Always ONE launch of the generic phase kernel's table instantiation (counted under CN_COUNT_ROLLOUT_KERNELS, never under
 * CN_COUNT_SCHEDULED_KERNELS); the fused small-crowd kernels and the 20-human shard kernel are not involved.
 * Refused before anything is enqueued: NULL e or actions, out with a required array NULL, n_steps < 0: CN_ERR_INVALID; a
 * CN_ROBOT_ORCA engine: CN_ERR_INVALID (use cn_rollout); an io that does not fit: as cn_rollout.  n_steps == 0: CN_OK, nothing
 * launched, nothing counted.  Asynchronous on the engine's stream: `actions` and the arrays of `out` must stay valid until the
 * launch has run. */
int cn_rollout_actions(cn_engine* e, const cn_rollout_io* io, int n_steps, const double* actions, const cn_trace_out* out);

/* ------------------------------------------------------------------------------------------------------
 * Multi-step lookahead (no version bump: a new symbol only).  CrowdSim.onestep_lookahead (crowd_sim.py:314-420 with
 * update=False; here cn_step(update=0)) answers "what if the robot takes action a now"; cn_lookahead_actions answers it for K
 * candidate SEQUENCES of n actions per env, in one launch, from the envs' current state and without touching it — what a
 * shooting or CEM planner scores.
 *   - Branch (b, k) starts from env b as it stands: agents, global time, heading, the humans present under `mixed`, and the
 *     kd-tree permutations of crowds above 10 humans (which no entry point copies into a second engine).
 *   - It applies actions[b][k][t] for t = 0, 1, .. exactly as cn_step(update=1) would — the humans react through ORCA — and
 *     stops after the first transition with done, or after n_steps.  Rows after a branch's end are not read.  Holonomic engines
 *     read a row as (vx, vy), CN_UNICYCLE engines as (v, r).
 *   - Nothing of the engine changes: no scenario ring, no auto-reset, no RNG draw, no record, no counter.  State, cn_rollout_io
 *     arrays, ring levels and cn_launch_counts are not written (the launch is NOT counted: CN_LAUNCH_COUNTERS keeps its length);
 *     a rollout in progress continues as if the call had not happened, and a pending lagged fill is not settled.
 *   - ret uses cn_set_gamma's table (cn_create installs gamma = 0.9, as for cn_rollout_begin), index 0 at the branch point;
 *     an engine without a table (a failed cn_set_gamma) is refused.
 * All arrays DEVICE memory; arrays of `out` are indexed [b][k]. */
typedef struct cn_lookahead_out {
    double*  ret;      /* [B][K] sum_t gamma^(t*dt*v_pref) * r_t, t = 0 at the branch point, left to right            */
    uint8_t* info;     /* [B][K] CN_* code of the LAST transition made: ReachGoal / Collision / Timeout = it ended there */
    int32_t* steps;    /* [B][K] transitions made, 1..n                                                                */
    double*  time;     /* [B][K] the env's global_time after the last transition made                                  */
    double*  final_state8; /* optional [B][K][A][8] state after the last transition made (cn_get_state layout)         */
    double*  final_theta;  /* optional [B][K]                                                                          */
} cn_lookahead_out;
/* ONE launch of the generic phase kernel's lookahead instantiation over B K virtual envs, on the engine's stream, whatever the
 * geometry.  Refused, in this order, before anything is enqueued: NULL actions, out, out->ret, out->info, out->steps or
 * out->time: CN_ERR_INVALID; n_steps < 0 or n_candidates < 1: CN_ERR_INVALID; NULL e: CN_ERR_INVALID; a CN_ROBOT_ORCA engine:
 * CN_ERR_INVALID; B K beyond a 32-bit env index or B K n beyond 2^59 rows: CN_ERR_UNSUPPORTED.  n_steps == 0: CN_OK, nothing
 * launched, nothing written.  Asynchronous: `actions` and the arrays of `out` must stay valid until the launch has run; `out`
 * itself is copied by the call. */
int cn_lookahead_actions(cn_engine* e, int n_steps, int n_candidates, const double* actions /* [B][K][n][2] */,
                         const cn_lookahead_out* out);

/* ------------------------------------------------------------------------------------------------------
 * Lookahead human model (no version bump: two new symbols; CN_LAUNCH_COUNTERS keeps its length).  How the humans of a
 * lookahead's branches move.  CN_HUMANS_ORCA (what cn_create installs): they react through ORCA, which reads every human's goal
 * — right inside this simulator, where the humans ARE ORCA.  CN_HUMANS_CONSTANT_VELOCITY: every human keeps the velocity it
 * has, the standard model of a planner fed observed positions and velocities; the reference's `[action_space] query_env =
 * false` (multi_human_rl.py:37-41, cadrl.py:104-110) carried from the one-step decision to the n-step lookahead.
 * A per-engine setting, read by cn_lookahead_actions and by everything that reaches a lookahead through it —
 * cn_lookahead_values, cn_plan_cem, cn_plan_rollout, cn_plan_mppi, cn_plan_mppi_rollout — and by nothing else: cn_step, every
 * cn_rollout_* call (the cn_rollout_step inside cn_plan_rollout / cn_plan_mppi_rollout too: the real step of a planner's closed
 * loop stays ORCA, only its model of the future changes) and cn_sarl_select do not look at it; cn_reset and the rollout calls
 * do not change it.  cn_lookahead_actions' refusals are the same under either model, in the same order, with the same messages. */
enum { CN_HUMANS_ORCA = 0, CN_HUMANS_CONSTANT_VELOCITY = 1 };
/* Refused before anything is touched: NULL e: CN_ERR_INVALID; a model that is neither value: CN_ERR_INVALID naming it. */
int cn_lookahead_set_human_model(cn_engine* e, int model);
/* NULL e or model_host: CN_ERR_INVALID. */
int cn_lookahead_get_human_model(const cn_engine* e, int* model_host);
/* Under CN_HUMANS_CONSTANT_VELOCITY branch (b, k) is the branch described above — the same start state, action rows, stop at
 * the first `done`, outputs, and nothing of the engine written — made of cn_step(update=1)'s transition with ONE substitution:
 * the velocity a human "chooses" is its own current float64 velocity (vx, vy), unrounded (under ORCA: the float32 ORCA result
 * widened to double).  All float64, every product and sum a separate IEEE operation in the order written, so that a host
 * restatement is bit-exact (a unicycle's cos / sin excepted: they are the device libm's).  Per step of a running branch, with
 * (px, py) the robot, dt = time_step, and t the transitions the branch has made:
 *   robot action   as under ORCA.  Holonomic: (ax, ay) = the row.  CN_UNICYCLE: row (v, r), th = theta + r,
 *                  (ax, ay) = (v cos(r + theta), v sin(r + theta)) for the collision test; the heading is carried.
 *   human slots    1 .. A - 1, every one, the parked placeholders of the `mixed` rule included: with (hx, hy), (hvx, hvy), r_h
 *                  the human's position, velocity and radius,
 *                    x1 = hx - px, y1 = hy - py, wx = hvx - ax, wy = hvy - ay, x2 = x1 + wx dt, y2 = y1 + wy dt,
 *                    sx = x2 - x1, sy = y2 - y1, u = clamp(((0 - x1) sx + (0 - y1) sy) / (sx sx + sy sy), 0, 1),
 *                    (cx, cy) = sx == 0 && sy == 0 ? (0 - x1, 0 - y1) : ((x1 + u sx) - 0, (y1 + u sy) - 0),
 *                    c = sqrt(fma(cy, cy, cx cx)) - r_h - r_robot        (the one fused operation)
 *   scan           in slot order: hit = c < 0; dmin = the smallest c seen BEFORE the first hit (infinity if none).
 *   robot end      holonomic (ex, ey) = (px + ax dt, py + ay dt); unicycle (px + cos(th) v dt, py + sin(th) v dt), products
 *                  left to right; reaching = sqrt(fma(ey - gy, ey - gy, (ex - gx) (ex - gx))) < r_robot.
 *   outcome        global_time >= time_limit - 1: Timeout, reward 0; else a hit: Collision, collision_penalty; else reaching:
 *                  ReachGoal, success_reward; else dmin < discomfort_dist: Danger, (dmin - discomfort_dist) *
 *                  discomfort_penalty_factor * dt, goes on; else Nothing, 0, goes on.
 *   book           ret <- ret + table[t] * reward (cn_set_gamma's table; 0 beyond its end), steps <- t + 1,
 *                  global_time <- global_time + dt.
 *   moves          robot <- (ex, ey), its velocity (ax, ay) — unicycle: theta <- python's th % (2 pi), velocity
 *                  (v cos(theta), v sin(theta)).  Human: hx <- hx + hvx dt, hy <- hy + hvy dt, one multiply and one add each,
 *                  sequential from step to step (never p0 + t dt v); its velocity, goal, radius and v_pref stay.
 * final_state8 / final_theta: the state after the branch's last transition, as under ORCA.  Neither robot_visible, the safety
 * spaces, max_neighbors, the kd-tree rows nor the humans' goals are read (the goals are copied into final_state8).
 * With n = 1 this is NOT cn_sarl_select's constant_velocity_model reward: that one is compute_reward on END positions
 * (multi_human_rl.py:65-90), this one the environment's SWEPT test — the environment's transition with the humans' policy
 * replaced, so `ret` means what it means under ORCA.  Humans do not stop at their goals.
 * One launch of a kernel of its own (lane = branch, the humans of an env shared by its K branches), not counted either. */

/* ------------------------------------------------------------------------------------------------------
 * Lookahead goal-progress term (no version bump: two new symbols; no struct, enum or counter touched).  A branch's return is
 * the environment's: +success on arrival, the collision penalty, the discomfort penalty, nothing else — so over a horizon that
 * does not reach the goal every collision-free candidate scores exactly 0.0 and a planner cannot tell which way the goal lies.
 * This setting adds the terminal term every MPC-style planner has: a weight on the progress the branch made towards the goal.
 * With w the engine's weight, (px0, py0) the robot's position as the engine state holds it when the launch runs, (gx, gy) its
 * goal, (px, py) its position after the branch's last transition — the one final_state8 reports, whether the branch ended or
 * ran the whole horizon — and norm2(x, y) = sqrt(fma(y, y, x * x)):
 *     d0   = norm2(px0 - gx, py0 - gy)
 *     d1   = norm2(px  - gx, py  - gy)
 *     ret' = ret + w * (d0 - d1)          one subtraction, one multiply, one add, in that order, float64, no fused operation
 * Added once, after the last reward of the branch, undiscounted, the same for every end code (a ReachGoal branch has
 * d1 < radius: the term is continuous across arrival).  With w != 0, ret' takes the place of ret wherever a lookahead reports
 * or uses it: out->ret of cn_lookahead_actions (both human models), cn_lookahead_paths, cn_lookahead_values and
 * cn_lookahead_paths_values; score = ret' + table[steps] * V of the two *_values calls; every per-mode ret_m of
 * cn_lookahead_modes, each at its own mode's last step with the robot's position after that step, before the reduction — hence
 * score, worst_mode and the per_mode rows; and so whatever the cn_plan_* calls rank, best_score and the MPPI weights, in every
 * planner form and every *_rollout closed loop.  Untouched: info, steps, time, final_state8, final_theta; the real steps inside
 * the closed loops (cn_rollout_step's rewards, the episode records, ep_return); cn_step, every rollout, cn_sarl_select's
 * one-step rewards.  Holonomic and CN_UNICYCLE engines and the `mixed` rule alike, wherever the call itself serves them.
 * The term is added inside the lookahead kernels, by instantiations of their own (their goal forms), which alone read w: with
 * w == 0.0 (what cn_create installs, or set back; -0.0 is 0.0) every call launches the kernels it launched before this setting
 * existed, and every output is bit for bit what it was.
 * A per-engine host-side setting: accepted on any engine, touches nothing on the device, survives cn_reset and the rollout
 * calls, like the human model above.
 * Refused before anything is touched, what depends on the argument alone first: a weight that is NaN, infinite or negative:
 * CN_ERR_INVALID with the value in the message (-0.0 is not negative: accepted, and means 0.0); NULL e: CN_ERR_INVALID. */
int cn_lookahead_set_goal_weight(cn_engine* e, double weight);        /* default 0.0 */
/* NULL e, then NULL weight_host: CN_ERR_INVALID. */
int cn_lookahead_get_goal_weight(const cn_engine* e, double* weight_host);

/* ------------------------------------------------------------------------------------------------------
 * Lookahead under predicted human motion (no version bump: four new symbols; no struct, enum or counter touched).  The two
 * human models above are the ends of a range: ORCA reads every human's goal, constant velocity extrapolates forever.  A planner
 * outside the simulator has a predictor of its own — a learned trajectory model, a goal-directed extrapolation, a recorded
 * track replayed — and cn_lookahead_paths scores action sequences against whatever it says: the caller hands over the velocity
 * every human takes at every step of the horizon.
 *   human_vel: DEVICE double [B][n_steps][A - 1][2].  human_vel[b][t][h] is the velocity (vx, vy) human slot h + 1 of env b
 *   takes during step t of the horizon; all K branches of env b share it.  Read as 16-byte words: align it to 16 bytes.
 * An ARGUMENT, not an engine setting: cn_lookahead_set_human_model's setting is neither read nor written by the four calls.
 * Branch (b, k) is exactly the branch of CN_HUMANS_CONSTANT_VELOCITY above with that section's ONE substitution made by the
 * table: the velocity a human "chooses" at step t is human_vel[b][t][h] (there: its own current velocity; under ORCA: the ORCA
 * result).  As in cn_step(update=1), a step distinguishes the velocity a human HAS when the step starts — (hvx, hvy) of its
 * state: the state velocity at t = 0, human_vel[b][t - 1][h] afterwards — from the one it chooses during it:
 *   the swept test      wx = hvx - ax, wy = hvy - ay with the velocity the human HAS, as crowd_sim.py:331-351 reads human.vx;
 *   the move            hx <- hx + cvx dt, hy <- hy + cvy dt with the chosen (cvx, cvy) = human_vel[b][t][h]: one multiply and
 *                       one add each, sequential from step to step; the chosen velocity becomes the one the human has;
 *   final_state8        the human's velocity columns hold human_vel[b][s][h], s the LAST step the branch made (steps - 1); its
 *                       position is the one after step s; goal, radius and v_pref are copied through as before.
 * Under constant velocity the two coincide, which is why that section names one velocity.  Everything else is that section's,
 * unchanged: the robot action (holonomic or CN_UNICYCLE), the one fused operation, the slot-order scan and the dmin rule, the
 * outcome priority, the book, theta.  Every slot 1 .. A - 1 takes part, the parked placeholders of the `mixed` rule
 * included: the caller writes zeros for them.  Rows behind the last step any branch of env b makes are not read.  Non-finite
 * velocities are NOT checked: a NaN or infinite row that a running branch uses makes its distances NaN, which compare false —
 * no collision, no danger — from there on.
 * A caller who holds predicted POSITIONS passes (p[t + 1] - p[t]) / dt; the ABI takes velocities so that two special cases are
 * bit-exact on every output: human_vel[b][t][h] = the state velocity for every t gives CN_HUMANS_CONSTANT_VELOCITY's result,
 * and the velocities recorded from ORCA humans that do not see the robot (robot_visible = 0; the state velocity after step t
 * of an engine whose robot is parked away from them) give CN_HUMANS_ORCA's.
 * cn_lookahead_paths refuses NULL human_vel first (CN_ERR_INVALID naming it), then everything cn_lookahead_actions refuses, in
 * its order and with its messages.  n_steps == 0: CN_OK, nothing launched, nothing written.  ONE launch (lane = branch, the
 * constant-velocity kernel's lane body), NOT counted; state, cn_rollout_io arrays, ring levels and cn_launch_counts are not
 * written, a rollout in progress continues as if the call had not happened.  Asynchronous: actions, human_vel and the arrays
 * of `out` must stay valid until the launch has run. */
int cn_lookahead_paths(cn_engine* e, int n_steps, int n_candidates,
                       const double* actions   /* [B][K][n][2] */,
                       const double* human_vel /* [B][n][A-1][2] */,
                       const cn_lookahead_out* out);
/* cn_lookahead_values (below) with cn_lookahead_paths as its lookahead: NULL human_vel first, then cn_lookahead_values'
 * refusals in its order (under this call's name where the message names the call), the same value and score. */
int cn_lookahead_paths_values(cn_engine* e, int n_steps, int n_candidates, const double* actions,
                              const double* human_vel, const cn_lookahead_out* out,
                              int sort_humans, float* value, double* score);
/* cn_plan_cem and cn_plan_mppi (below, with their structs) scoring through cn_lookahead_paths — cn_lookahead_paths_values with
 * cfg->bootstrap —: NULL human_vel first, then every refusal of the cn_plan_* calls; the draw, refit and MPPI update are
 * untouched, human_vel is [B][cfg->n_steps][A - 1][2].  There is deliberately no *_rollout form: a prediction is made from the
 * state after each real step, so the closed loop goes through the host once per step (cn_plan_cem_paths, cn_rollout_step,
 * cn_plan_shift). */
typedef struct cn_plan_cfg cn_plan_cfg;
typedef struct cn_plan cn_plan;
int cn_plan_cem_paths (cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan,
                       const double* human_vel, uint32_t counter);
int cn_plan_mppi_paths(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan,
                       const double* human_vel, double temperature, int fit_std, uint32_t counter);
/* (That holds for a predictor of the CALLER's.  For the two predictors the library ships on the device — cn_predict, at the end
 * of this header — the closed loop is one call: cn_plan_cem_predict_rollout / cn_plan_mppi_predict_rollout.) */

/* ------------------------------------------------------------------------------------------------------
 * Lookahead under several predicted futures (no version bump: three new symbols, two new structs, one new enum; no existing
 * struct, enum or counter touched).  A predictor seldom returns one future: a learned trajectory model returns M weighted
 * modes, a cautious planner holds "keeps walking" beside "heads for its goal".  cn_lookahead_modes scores every branch (b, k)
 * against M tables at once and reduces the M returns to the number such a planner optimises: the expected return, the worst
 * case, either one less a penalty on the probability of a collision.  The robot of a branch does not depend on the humans (its
 * actions are open-loop), so ONE launch moves it once and tests it against the M sets of humans: the action table is read once,
 * where M cn_lookahead_paths calls read it M times.
 *   human_vel: DEVICE double [B][M][n_steps][A - 1][2]: human_vel[b][m] is cn_lookahead_paths' table of env b under mode m.  Read
 *              as 16-byte words: align it to 16 bytes.
 *   weight:    DEVICE double [B][M], or NULL = every weight 1.0 / (double)M.  Used as given: not normalised, not validated.
 * Per-mode branch.  Mode m of branch (b, k) is exactly cn_lookahead_paths' branch (b, k) with the table human_vel[b][m], bit
 * for bit on ret, info, steps and time: the section above holds unchanged — holonomic and CN_UNICYCLE engines, the parked
 * slots of the `mixed` rule, the velocity a human HAS against the one it chooses, non-finite velocities NOT checked.  Each mode
 * ends at its own first `done`; Timeout and ReachGoal depend on the robot alone and so end every mode still running at that
 * step.  Action rows behind the step at which a branch's last mode ends are not read, nor are table rows behind the last step
 * any branch of env b makes.
 * Reduction, per branch, float64, every product and sum a separate IEEE operation, sequential in m from 0.0; w_m = weight[b][m]:
 *   r          CN_MODES_MEAN: sum_m w_m * ret_m.   CN_MODES_MIN: min_m ret_m (weights are not read for it).
 *   risk       sum_m w_m * (info_m == Collision ? 1.0 : 0.0)
 *   score      r - risk_penalty * risk
 *   worst_mode the smallest m that holds the lowest ret_m; worst_info, worst_steps, worst_time: that mode's values.
 * There is no final_state8, no final_theta and no bootstrap form: they belong to the per-(branch, mode) state, M times the
 * largest array of cn_lookahead_paths. */
enum { CN_MODES_MEAN = 0, CN_MODES_MIN = 1 };
typedef struct cn_path_modes {
    int32_t n_modes;          /* M: 1 .. 8                                                  */
    int32_t reduce;           /* CN_MODES_MEAN | CN_MODES_MIN                               */
    double  risk_penalty;     /* finite, >= 0                                               */
    const double* human_vel;  /* DEVICE [B][M][n_steps][A-1][2], 16-byte aligned            */
    const double* weight;     /* DEVICE [B][M], or NULL = every weight 1.0 / (double)M      */
} cn_path_modes;
typedef struct cn_modes_out { /* all DEVICE memory                                          */
    double*  score;       /* [B][K]    required                                             */
    double*  risk;        /* [B][K]    optional                                             */
    int32_t* worst_mode;  /* [B][K]    optional                                             */
    uint8_t* worst_info;  /* [B][K]    optional                                             */
    int32_t* worst_steps; /* [B][K]    optional                                             */
    double*  worst_time;  /* [B][K]    optional                                             */
    double*  ret;         /* [B][K][M] optional per-mode rows: cn_lookahead_out's, per mode */
    uint8_t* info;        /* [B][K][M] optional                                             */
    int32_t* steps;       /* [B][K][M] optional                                             */
    double*  time;        /* [B][K][M] optional                                             */
} cn_modes_out;
/* Refused, in this order, before anything is enqueued: NULL modes, modes->human_vel, out or out->score: CN_ERR_INVALID naming
 * it; n_modes < 1: CN_ERR_INVALID, n_modes > 8: CN_ERR_UNSUPPORTED with the number; a reduce that is neither value:
 * CN_ERR_INVALID naming it; a risk_penalty that is negative or not finite: CN_ERR_INVALID; everything cn_lookahead_actions
 * refuses for (n_steps, n_candidates, actions), in its order and with its messages; B K M beyond an int: CN_ERR_UNSUPPORTED.
 * n_steps == 0: CN_OK, nothing launched, nothing written.  ONE launch of a kernel of its own (lane = branch, the M H humans of an
 * env shared by its K branches), NOT counted in cn_launch_counts; state, cn_rollout_io arrays, ring levels and the human-model
 * setting are neither read nor written, a rollout in progress continues as if the call had not happened.  Asynchronous on the
 * engine's stream: actions, human_vel, weight and the arrays of `out` must stay valid until the launch has run; `modes` and
 * `out` themselves are copied by the call. */
int cn_lookahead_modes(cn_engine* e, int n_steps, int n_candidates, const double* actions /* [B][K][n][2] */,
                       const cn_path_modes* modes, const cn_modes_out* out);
/* cn_plan_cem and cn_plan_mppi (below) scoring through cn_lookahead_modes: plan->look.ret receives `score`, plan->look.info,
 * look.steps and look.time the worst mode's rows; the draw, refit, MPPI update and cn_plan_shift are untouched and rank
 * look.ret.  human_vel is [B][M][cfg->n_steps][A - 1][2].  Refused: NULL modes first; then every refusal of the cn_plan_* calls;
 * then cfg->bootstrap != 0: CN_ERR_UNSUPPORTED naming bootstrap; then cn_lookahead_modes' refusals.  No *_rollout form, for the
 * reason given above; a CN_UNICYCLE engine without cn_plan_set_unicycle stays refused as by every cn_plan_* call. */
int cn_plan_cem_modes (cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const cn_path_modes* modes, uint32_t counter);
int cn_plan_mppi_modes(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const cn_path_modes* modes,
                       double temperature, int fit_std, uint32_t counter);
/* (Several futures made by the device predictors: cn_predictors with n_modes > 1, cn_plan_*_predict_rollout below.) */

/* ------------------------------------------------------------------------------------------------------
 * Value-bootstrapped lookahead (no version bump: new symbols only).  The n-step return a value-network policy means,
 *   score = sum_{t<n} gamma^(t dt v_pref) r_t + gamma^(n dt v_pref) V(s_n)
 * (MultiHumanRL.predict, multi_human_rl.py:52, is n = 1; Explorer.update_memory's TD targets train V to mean it), needs V of
 * states the engine does not hold: a lookahead's branch ends, the rows of a recorded trace, states made up for analysis. */
/* V(state) of n joint states the CALLER holds in the env layout: state8 double [n][A][8] (cn_get_state's rows),
 * theta double [n] (robot heading; read only by CN_UNICYCLE engines, where it is required; NULL otherwise allowed).
 * Rows = MultiHumanRL.transform of each state (rotate of float32 [robot full state | human h], cadrl.py:187-222) —
 * the rows cn_sarl_transform writes for the engine's own state; sort_humans as in cn_sarl_transform.
 * value float [n].  The engine's env state is neither read nor written. */
int cn_sarl_state_values(cn_engine* e, const double* state8, const double* theta, int64_t n, int sort_humans, float* value);
/* Any n >= 1: the states go through the engine's network buffers in passes of at most num_envs x n_actions, on the kernel family
 * cn_sarl_configure chose (cn_sarl_network_route; CN_PRECISION_F16X2 engines included) — every model and human count that route
 * takes; on a narrow-route engine the narrow kernel reads the rows (as for cn_sarl_values), CN_MODEL_CADRL there runs the
 * configuration's one-tile LDS kernel.  A state's value does not depend on n or on its place among the n.  No allocation after
 * the first call.  Refused, in this order, before anything is enqueued: NULL state8, NULL value, n < 1, NULL e, not configured or
 * no weights set, theta == NULL on a CN_UNICYCLE engine: CN_ERR_INVALID; an engine with occupancy maps (with_om: the maps of
 * arbitrary states are not built on the device), an engine under the `mixed` rule: CN_ERR_UNSUPPORTED.  Side effects: the
 * buffers cn_sarl_export reads (V, X) may be overwritten — export what a cn_sarl_select left BEFORE calling this; a launch on
 * the narrow tiles counts under CN_COUNT_SARL_NARROW, one per pass; the humans' ORCA velocities cn_sarl_sample_step keeps are
 * forgotten, as by every other entry point.  Nothing else of the engine changes.  Asynchronous on the engine's stream. */

/* cn_lookahead_actions(e, n_steps, n_candidates, actions, out) followed by the bootstrap, in one call:
 *   value float  [B][K]  V of the state after the branch's last transition (every branch, ended or not)
 *   score double [B][K]  ret + (info is ReachGoal / Collision / Timeout ? 0 : table[steps] * (double)value),
 *                        table = cn_set_gamma's, the one `ret` uses; one multiply and one add, in that order
 * out->final_state8 must be non-NULL (and out->final_theta on CN_UNICYCLE engines): the caller owns the branch states. */
int cn_lookahead_values(cn_engine* e, int n_steps, int n_candidates, const double* actions, const cn_lookahead_out* out,
                        int sort_humans, float* value, double* score);
/* An ended branch gets no bootstrap — the TD target of an episode's last transition is the reward alone (explorer.py:107-113) —
 * but its value is written, for the caller who wants multi_human_rl.py:52's decision-time form.  Refused before anything is
 * enqueued: everything cn_lookahead_actions refuses, in its order and with its messages; then NULL out->final_state8, value,
 * score: CN_ERR_INVALID; then cn_sarl_state_values' conditions on the engine, in its order.  n_steps == 0: CN_OK, nothing
 * launched, nothing written.  State, rollout io, ring levels and launch counters are left as cn_lookahead_actions leaves them,
 * apart from CN_COUNT_SARL_NARROW and cn_sarl_export's buffers (above). */

/* ------------------------------------------------------------------------------------------------------
 * Device CEM planner (no version bump: new symbols only).  The caller cn_lookahead_actions / cn_lookahead_values were built
 * for: per env a Gaussian over sequences of n actions (mean, std per step and component), from which K candidates are drawn,
 * scored by the lookahead, ranked, and the distribution refitted to the E best (cross-entropy method), I times per real step;
 * the best sequence's first action is taken, and the plan shifted by one step — or re-seeded where an episode ended.  Drawing,
 * ranking, refitting, shifting and the closed loop run on the device, enqueued on the engine's stream; no call synchronises.
 * CN_ROBOT_EXTERNAL engines: a holonomic robot, action rows (vx, vy); a CN_UNICYCLE engine is CN_ERR_UNSUPPORTED until
 * cn_plan_set_unicycle (below, "Unicycle planners") has named its rotation bound, and then planned with rows (v, r).  All arrays
 * are DEVICE memory, caller-owned, and must stay valid until the work has run; cfg and plan themselves are copied by the call.  Action
 * rows (mean, std, best_actions, action, candidates) are read and written as 16-byte words: align them to 16 bytes.
 *
 * The arithmetic below is float64, every product and sum a separate IEEE operation in the order written, so that a host
 * restatement is bit-exact (the draw's log / cos / sin excepted: they are the device libm's).  v_pref is the robot's, read
 * from its row of the engine state.  Scores are finite by construction: NaN is NOT handled. */
typedef struct cn_plan_cfg {
    int32_t n_steps;      /* n, horizon: 1 .. 256 (kMaxDiscount)                       */
    int32_t n_candidates; /* K: 2 .. 1024                                              */
    int32_t n_elites;     /* E: 1 .. min(K, 64)                                        */
    int32_t iterations;   /* I >= 1 CEM iterations per planning step                   */
    int32_t bootstrap;    /* 0: rank by look.ret; 1: by cn_lookahead_values' score     */
    int32_t sort_humans;  /* passed to cn_lookahead_values                             */
    double  init_std;     /* > 0, finite (velocity units)                              */
    double  min_std;      /* >= 0, finite                                              */
    double  smoothing;    /* alpha in [0, 1)                                           */
    uint64_t seed;
} cn_plan_cfg;

typedef struct cn_plan {
    double* mean;          /* [B][n][2] in/out                                          */
    double* std;           /* [B][n][2] in/out                                          */
    double* best_actions;  /* [B][n][2] out                                             */
    double* best_score;    /* [B] out                                                   */
    double* action;        /* [B][2] out = best_actions[b][0]                           */
    double* candidates;    /* [B][K][n][2]: after a call, the LAST iteration's          */
    cn_lookahead_out look; /* [B][K] rows of the last iteration; final_state8 required iff bootstrap */
    float*  value;         /* [B][K], required iff bootstrap                            */
    double* score;         /* [B][K], required iff bootstrap                            */
    int32_t* order;        /* optional [B][K]: candidate index at rank r, last iteration */
} cn_plan;

/* Every cn_plan_* call refuses, in this order and before anything is enqueued: NULL cfg, plan or a required array (everything
 * of cn_plan but `order`; look.final_state8, value and score iff cfg->bootstrap): CN_ERR_INVALID with the name; cfg out of the
 * ranges above: CN_ERR_INVALID — n_candidates > 1024, n_elites > 64 and n_steps > 256: CN_ERR_UNSUPPORTED with the number;
 * NULL engine or a CN_ROBOT_ORCA engine: CN_ERR_INVALID; a CN_UNICYCLE engine without cn_plan_set_unicycle: CN_ERR_UNSUPPORTED;
 * then whatever
 * cn_lookahead_actions refuses for (n_steps, n_candidates, candidates, look) and, with bootstrap, cn_lookahead_values, with
 * their messages; cn_plan_shift and cn_plan_rollout then what cn_rollout_step refuses for the io block. */

/* The goal-directed prior, for every env with mask == NULL || mask[b] (mask: DEVICE uint8 [B]): with (px, py), (gx, gy) the
 * robot's position and goal as the engine state holds them,
 *   dx = gx - px, dy = gy - py, dist = sqrt(dx dx + dy dy), speed = min(v_pref, dist / time_step)
 *   mean[b][t] = dist > 0 ? ((dx / dist) speed, (dy / dist) speed) : (0, 0)   for every t;   std[b][t][c] = init_std */
int cn_plan_reset(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const uint8_t* mask /* [B] or NULL = all */);
/* candidates[b][k][t], one lane per row, one 16-byte store per row.  k = 0: the mean itself.  k >= 1: mean[b][t] + std[b][t] *
 * (z0, z1) componentwise, (z0, z1) ONE Box-Muller pair from ONE Philox4x32-10 block with counter words (t, k, b, counter) and
 * key (seed & 0xffffffff, seed >> 32) — so a row depends on neither B, K nor n.  With w0..w3 the block's words:
 *   u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) / 2^53  in (0, 1],   u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) / 2^53
 *   r = sqrt(-2 log(u1)),  z0 = r cos(2 pi u2),  z1 = r sin(2 pi u2)
 * Every row, k = 0 included, is then clipped to the robot's speed: nrm = sqrt(ax ax + ay ay); if nrm > v_pref, s = v_pref /
 * nrm, ax *= s, ay *= s. */
int cn_plan_draw(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter);
/* One 64-lane workgroup per env.  s_k = bootstrap ? score[b][k] : look.ret[b][k];  rank(k) = #{j : s_j > s_k, or s_j == s_k
 * and j < k};  order[b][rank(k)] = k if order is given.  With k* the rank-0 candidate: if !keep_best || s_k* > best_score[b]
 * (strict: the earliest holder wins), best_actions[b] = candidates[b][k*], best_score[b] = s_k*, action[b] = best_actions[b][0].
 * The elites are ranks 0 .. E - 1; per component (t, c), both sums sequential in rank order from 0.0:
 *   m = (sum_e a_e) / E,  var = (sum_e (a_e - m) (a_e - m)) / E,  sd = sqrt(var)
 *   mean <- smoothing mean + (1.0 - smoothing) m,   std <- max(min_std, smoothing std + (1.0 - smoothing) sd) */
int cn_plan_refit(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, int keep_best);
/* One planning step: for i in 0 .. iterations - 1: cn_plan_draw(counter + i); cn_lookahead_actions(e, n_steps, n_candidates,
 * candidates, &look) — cn_lookahead_values(.., sort_humans, value, score) with bootstrap —; cn_plan_refit(keep_best = i > 0).
 * The engine is left exactly as those lookahead calls leave it: no state, io, ring or counter changes beyond what
 * cn_lookahead_values documents; the plan kernels are NOT counted in cn_launch_counts (CN_LAUNCH_COUNTERS keeps its length). */
int cn_plan_cem(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter);
/* After a real step (cn_rollout_step) of the rollout `io` describes.  An env with io->active[b] == 0: nothing.  An env with
 * io->cur_steps[b] == 0 — its episode has just ended and the next scenario is loaded — gets cn_plan_reset's prior from the
 * state as it now stands; an env still WAITING for a scenario has cur_steps == 0 as well and gets the prior of its stale state.
 * Every other env: mean[b][t] <- mean[b][t + 1] for t < n - 1, mean[b][n - 1] stays, std <- init_std everywhere.  In place. */
int cn_plan_shift(cn_engine* e, const cn_rollout_io* io, const cn_plan_cfg* cfg, const cn_plan* plan);
/* The closed loop, one C call without host work or synchronisation between the steps: for s in 0 .. n_real_steps - 1:
 * cn_plan_cem(counter + s * iterations); cn_rollout_step(e, io, plan->action); cn_plan_shift — through those functions' own host
 * paths, so the checks, the scenario-ring fill and the launch counters are exactly as if the caller had made the calls.
 * n_real_steps < 0: CN_ERR_INVALID; n_real_steps == 0: CN_OK, nothing enqueued. */
int cn_plan_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                    uint32_t counter);

/* ------------------------------------------------------------------------------------------------------
 * Device MPPI update (no version bump: three new symbols, the structs above unchanged).  The other standard update of a
 * sampling-based planner, beside the CEM refit and over the same cn_plan_cfg / cn_plan: EVERY candidate contributes, weighted by
 * the softmax of its score at `temperature`, and the action taken is the updated mean's first row, not the best sample's.
 * n_elites is range-checked as in every cn_plan_* call but not read.  The three calls refuse what every cn_plan_* call
 * refuses, in that order and with their own names; and, after the cfg ranges and before the engine is looked at, a
 * temperature that is not finite or <= 0: CN_ERR_INVALID naming `temperature`.
 *
 * One 64-lane workgroup per env, float64, every product and sum a separate IEEE operation in the order written (a host
 * restatement is bit-exact but for exp, which is the device libm's).  s_k, rank(k), order and k* as in cn_plan_refit; if
 * !keep_best || s_k* > best_score[b] (strict), best_actions[b] = candidates[b][k*] and best_score[b] = s_k*.  With s_max = s_k*:
 *   w_k = exp((s_k - s_max) / temperature)   (so w_k* = 1),   Z = sum_k w_k   (so Z >= 1)
 * per component (t, c), with a_k = candidates[b][k][t][c]; Z and both sums sequential in k order from 0.0:
 *   num = sum_k w_k a_k,  m = num / Z,  var = (sum_k w_k ((a_k - m) (a_k - m))) / Z,  sd = sqrt(var)
 *   mean <- smoothing mean + (1.0 - smoothing) m
 *   std  <- max(min_std, smoothing std + (1.0 - smoothing) sd)   only if fit_std; otherwise std is not touched (classic MPPI:
 *           a fixed sampling deviation, which cn_plan_shift sets back to init_std as for CEM)
 * action[b] = the updated mean[b][0], clipped by cn_plan_draw's rule with the robot's v_pref — NOT best_actions[b][0].
 * NaN scores are not handled, as in cn_plan_refit. */
int cn_plan_mppi_update(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, double temperature, int fit_std, int keep_best);
/* One planning step: for i in 0 .. iterations - 1: cn_plan_draw(counter + i); cn_lookahead_actions — cn_lookahead_values with
 * bootstrap —; cn_plan_mppi_update(keep_best = i > 0).  The engine is left exactly as those lookahead calls leave it. */
int cn_plan_mppi(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, double temperature, int fit_std, uint32_t counter);
/* cn_plan_rollout with the other update: for s in 0 .. n_real_steps - 1: cn_plan_mppi(counter + s * iterations);
 * cn_rollout_step(e, io, plan->action); cn_plan_shift — one C call, no host work or synchronisation between the steps.
 * n_real_steps < 0: CN_ERR_INVALID; n_real_steps == 0: CN_OK, nothing enqueued. */
int cn_plan_mppi_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,
                         double temperature, int fit_std, uint32_t counter);

/* ------------------------------------------------------------------------------------------------------
 * Unicycle planners (no version bump: two new symbols; cn_plan_cfg, cn_plan and CN_LAUNCH_COUNTERS unchanged).  A unicycle
 * robot's action is ActionRot (v, r): a speed and a rotation.  How far it may turn per step is the caller's choice, not a fact
 * of the environment (the reference puts it in the policy's action space: +-pi/4), and v and r have different units, so the
 * plan needs a rotation bound R and a second initial deviation.  cn_plan_set_unicycle names both and OPTS THE ENGINE IN: until
 * it has been called, every cn_plan_* call refuses a CN_UNICYCLE engine as before (CN_ERR_UNSUPPORTED, at the same place of the
 * refusal order, nothing enqueued); afterwards every cn_plan_* call serves it — reset, draw, refit, cem, shift, rollout, the
 * MPPI calls, the *_paths and *_modes planners and every *_predict_*rollout — with action rows (v, r) in mean, std, candidates,
 * best_actions and action.  A host-side setting like cn_lookahead_set_goal_weight: it survives cn_reset, cannot be unset (the
 * engine's lifetime is its scope), and the getter gives (0, 0) until it is made.  The setter refuses, in this order: NULL
 * engine; max_rotation not finite, <= 0 or > pi; init_std_rotation not finite or <= 0; an engine that is not CN_UNICYCLE, or is
 * CN_ROBOT_ORCA (the setting would never be read): all CN_ERR_INVALID, the middle two naming the argument.
 *
 * The arithmetic on such an engine, float64, one IEEE operation per product and sum in the order written, with R = max_rotation:
 *   clip   (in place of the speed-disc rule, in cn_plan_draw and for cn_plan_mppi_update's action; every row, k = 0 included)
 *            v <- v < 0 ? 0 : (v > v_pref ? v_pref : v)         (no reverse gear)
 *            r <- r < -R ? -R : (r > R ? R : r)
 *   draw   the same Philox block and Box-Muller pair: v = mean.v + std.v z0, r = mean.r + std.r z1, then the clip
 *   prior  (cn_plan_reset; cn_plan_shift where cur_steps == 0) a recurrence in t from the robot's (px, py), its goal and its
 *          heading th = theta[b] as the engine holds them; per t:
 *            dx = gx - px, dy = gy - py, dist = sqrt(dx dx + dy dy), speed = min(v_pref, dist / time_step)
 *            if !(dist > 0): mean[b][t] = (0, 0), nothing moves
 *            else: bearing = atan2(dy, dx), d = bearing - th, turn = d - 2 pi floor((d + pi) / (2 pi))   (in [-pi, pi))
 *                  r = turn < -R ? -R : (turn > R ? R : turn),  mean[b][t] = (speed, r),  th <- th + r
 *                  px <- px + cos(th) speed time_step,  py <- py + sin(th) speed time_step   (the step's own end point)
 *          std[b][t] = (cfg->init_std, init_std_rotation); cn_plan_shift writes that pair on every env it shifts, too
 *          (atan2 / cos / sin are the device libm's: a host restatement agrees to the last bits, not bit for bit)
 *   refit, MPPI sums   component-wise, unchanged: r stays within [-R, R], so no angle wraps; min_std floors both components
 *   nominal rollouts   candidate 0 of the first draw is the clipped mean in (v, r), which cn_predict_orca_robot follows from the
 *                      engine's heading */
int cn_plan_set_unicycle(cn_engine* e, double max_rotation, double init_std_rotation);
int cn_plan_get_unicycle(cn_engine* e, double* max_rotation, double* init_std_rotation);   /* (0, 0) until set */

/* ------------------------------------------------------------------------------------------------------
 * Device predictors and the closed loop on predicted futures (no version bump: three new symbols, one new struct, one new enum;
 * no existing struct, enum or counter touched).  cn_lookahead_paths / cn_lookahead_modes take the humans' predicted velocities
 * from the caller, and a caller with a predictor of their own keeps the per-step calls above.  The two predictors the project
 * ships (crowdnav_amd/predict.py: constant_velocity, to_goal) are a few float64 operations per human and step; cn_predict makes
 * their tables on the device from the engine's state as it stands, which is what lets the whole closed loop — predict, plan,
 * real step, shift — run without the host.
 *   human_vel: DEVICE double [B][M][n_steps][A - 1][2], written as 16-byte words (align it to 16 bytes).  M = 1: exactly
 *   cn_lookahead_paths' table; M > 1: cn_lookahead_modes', mode m made by models[m].
 * One lane per (b, m, h): it reads position, velocity, goal and v_pref of human slot h + 1 of env b once and walks t = 0 ..
 * n_steps - 1.  Float64, every product, quotient and sum a separate IEEE operation in the order written, sqrt correctly rounded, so
 * that predict.py on a host copy of the state (cn_get_state) restates the table bit for bit:
 *   CN_PREDICT_CONSTANT_VELOCITY  human_vel[b][m][t][h] = the human's state velocity, for every t.
 *   CN_PREDICT_TO_GOAL            with (px, py) the human's position at first, dt the engine's time_step, per step t:
 *                                   dx = gx - px, dy = gy - py, dist = sqrt(dx dx + dy dy)
 *                                   v = (0, 0)                                    if !(dist > 0)
 *                                       (dx / dt, dy / dt)                        else if dist <= v_pref dt  (lands on the goal)
 *                                       ((dx / dist) v_pref, (dy / dist) v_pref)  otherwise
 *                                   human_vel[b][m][t][h] = v;  px <- px + vx dt, py <- py + vy dt
 * The parked placeholders of the `mixed` rule stand at their goals with zero velocity: both models give them zeros.
 * cn_predict serves ANY engine (CN_ROBOT_ORCA and CN_UNICYCLE included: only the humans are read).  ONE launch on the engine's
 * stream, NOT counted in cn_launch_counts; state, cn_rollout_io arrays, ring levels and the human-model setting are not
 * written, a rollout in progress continues as if the call had not happened.  Refused, in this order, before anything is
 * enqueued: NULL models, NULL human_vel: CN_ERR_INVALID naming it; n_modes < 1: CN_ERR_INVALID, n_modes > 8: CN_ERR_UNSUPPORTED
 * with the number; a model that is neither value: CN_ERR_INVALID naming its index and the value; n_steps < 0: CN_ERR_INVALID;
 * NULL engine: CN_ERR_INVALID; B M n_steps (A - 1) rows beyond an int: CN_ERR_UNSUPPORTED.  n_steps == 0: CN_OK, nothing
 * launched, nothing written.  Asynchronous: human_vel must stay valid until the launch has run; `models` is copied by the call. */
enum { CN_PREDICT_CONSTANT_VELOCITY = 0, CN_PREDICT_TO_GOAL = 1 };
int cn_predict(cn_engine* e, int n_steps, int n_modes,
               const int32_t* models /* HOST [n_modes] */,
               double* human_vel     /* DEVICE [B][M][n][A-1][2], 16-byte aligned */);

typedef struct cn_predictors {      /* 64 bytes */
    int32_t n_modes;        /* M: 1 .. 8                                    offset 0  */
    int32_t model[8];       /* CN_PREDICT_* of mode m; entries >= M not read       4  */
    int32_t reduce;         /* CN_MODES_MEAN | CN_MODES_MIN; read when M > 1      36  */
    double  risk_penalty;   /* finite, >= 0; read when M > 1                      40  */
    double* human_vel;      /* DEVICE scratch [B][M][cfg->n_steps][A-1][2]        48  */
    const double* weight;   /* DEVICE [B][M] or NULL = 1/M each; read when M > 1  56  */
} cn_predictors;
/* cn_plan_rollout / cn_plan_mppi_rollout against the device predictors: for s in 0 .. n_real_steps - 1:
 *   cn_predict(e, cfg->n_steps, M, pred->model, pred->human_vel);
 *   M == 1: cn_plan_cem_paths / cn_plan_mppi_paths(.., pred->human_vel, counter + s * iterations) — cfg->bootstrap is served,
 *           through cn_lookahead_paths_values;
 *   M > 1:  cn_plan_cem_modes / cn_plan_mppi_modes with {M, reduce, risk_penalty, human_vel, weight} and that counter;
 *   cn_rollout_step(e, io, plan->action); cn_plan_shift
 * — one C call, no host work or synchronisation between the steps, bit for bit what those calls give.  An env whose episode
 * has just ended is predicted from its new scenario; one still waiting for a scenario from its stale state, as cn_plan_shift
 * seeds its prior from it.  After the call pred->human_vel holds the table the LAST planning step scored against.  Refused, in
 * this order, before anything is enqueued: NULL pred, NULL pred->human_vel: CN_ERR_INVALID naming it; n_modes and the models as
 * by cn_predict; everything cn_plan_rollout / cn_plan_mppi_rollout refuses, in their order (CN_ROBOT_ORCA engines,
 * and CN_UNICYCLE ones without cn_plan_set_unicycle, stay refused, as by every cn_plan_* call); for M > 1 cfg->bootstrap != 0: CN_ERR_UNSUPPORTED naming bootstrap, then
 * cn_lookahead_modes' refusals; the table's rows beyond an int: CN_ERR_UNSUPPORTED.  n_real_steps == 0: CN_OK, nothing enqueued. */
int cn_plan_cem_predict_rollout (cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                 const cn_plan* plan, const cn_predictors* pred, uint32_t counter);
int cn_plan_mppi_predict_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                 const cn_plan* plan, const cn_predictors* pred, double temperature, int fit_std,
                                 uint32_t counter);

/* ------------------------------------------------------------------------------------------------------
 * The ORCA predictor: humans that avoid each other, the robot unseen (no version bump: three new symbols; no existing struct,
 * enum or counter touched — it is not a CN_PREDICT_* value, because its kernel is of another kind: a workgroup per env, not a
 * lane per human).  It sits between the two predictors above, whose humans walk through each other, and cn_lookahead_actions
 * under CN_HUMANS_ORCA, whose humans react to each of the K candidate robot paths: its result does not depend on the robot's
 * candidate, so it is made once per env and every *_paths / *_modes call can use it.
 *   cn_predict_orca writes slot `mode` of a table laid out as cn_predict's — human_vel [B][n_modes][n_steps][A - 1][2] — and no
 *   other slot: n_modes = 1, mode = 0 is cn_lookahead_paths' table; with n_modes > 1 it fills one future of a cn_lookahead_modes
 *   table whose other slots cn_predict or the caller made.
 * What the table means: from the engine's state as it stands the humans are stepped n_steps times exactly as cn_step steps them
 * on an engine with robot_visible = 0 and freshly made simulators (cn_drop_sims): every human solves ORCA against the other
 * humans only, with the engine's own ORCA parameters, max_neighbors, time_step and radii; human_vel[b][mode][t][h] is the float32
 * velocity human h + 1 chooses at step t — what cn_step reports in orca_vel — widened to double; the human then moves by
 * p + v dt in float64 (product and sum separate operations) and keeps that velocity as its current one for the next solve.
 * The robot is not stepped, tested or read; there are no rewards and no episode end: all n_steps rows are always written.  On
 * the kd route (A > 10) the simulators' visiting order starts as a fresh simulator's and is carried through the n steps inside
 * the kernel; the engine's own kd rows are neither read nor written.  The parked placeholders of the `mixed` rule get what
 * cn_step's orca_vel gives them.  It is the humans' policy itself: on an engine whose humans do not see the robot,
 * cn_lookahead_paths with this table is cn_lookahead_actions under CN_HUMANS_ORCA, bit for bit (fresh simulators on both sides).
 * cn_predict_orca serves ANY engine (CN_ROBOT_ORCA, CN_UNICYCLE and robot_visible = 1 included).  ONE launch on the engine's
 * stream — step_kernel's workgroup per E envs, under the engine's Params with robot_visible = 0 and robot_orca = 0 — NOT counted
 * in cn_launch_counts; state, cn_rollout_io arrays, ring levels, the human-model setting, the robot's captured simulator and the
 * kd rows are not written, a rollout in progress continues as if the call had not happened.  Refused, in this order, before
 * anything is enqueued: NULL human_vel: CN_ERR_INVALID; n_modes < 1: CN_ERR_INVALID, n_modes > 8: CN_ERR_UNSUPPORTED with the
 * number; mode outside 0 .. n_modes - 1: CN_ERR_INVALID with both numbers; n_steps < 0: CN_ERR_INVALID; NULL engine:
 * CN_ERR_INVALID; B n_modes n_steps (A - 1) rows beyond an int: CN_ERR_UNSUPPORTED.  n_steps == 0: CN_OK, nothing launched,
 * nothing written.  Asynchronous: human_vel must stay valid until the launch has run. */
int cn_predict_orca(cn_engine* e, int n_steps, int n_modes, int mode,
                    double* human_vel /* DEVICE [B][n_modes][n_steps][A-1][2], 16-byte aligned */);
/* cn_plan_*_predict_rollout with one future made by cn_predict_orca: per real step exactly their sequence, and after cn_predict
 * has written the table
 *   cn_predict_orca(e, cfg->n_steps, M, orca_mode, pred->human_vel)
 * overwrites slot orca_mode; then the paths planner (M == 1) or the modes planner (M > 1), cn_rollout_step and cn_plan_shift —
 * one C call, no host work or synchronisation between the steps, bit for bit what those calls give.  pred->model[orca_mode]
 * must still be a valid CN_PREDICT_* value: it is computed and overwritten (a launch of a few microseconds); struct
 * cn_predictors and its checks are as above.  Refused, before anything is enqueued: everything cn_plan_*_predict_rollout
 * refuses, in their order and with this call's name, and — after the models, before the engine is looked at — orca_mode
 * outside 0 .. M - 1: CN_ERR_INVALID with both numbers.  CN_ROBOT_ORCA engines, and CN_UNICYCLE ones without
 * cn_plan_set_unicycle, stay refused, as by every cn_plan_* call, and so does M > 1 with cfg->bootstrap. */
int cn_plan_cem_predict_orca_rollout (cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                      const cn_plan* plan, const cn_predictors* pred, int orca_mode, uint32_t counter);
int cn_plan_mppi_predict_orca_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                      const cn_plan* plan, const cn_predictors* pred, int orca_mode, double temperature,
                                      int fit_std, uint32_t counter);

/* ------------------------------------------------------------------------------------------------------
 * The ORCA predictor with the robot in sight, on its nominal plan (no version bump: three new symbols; no existing struct, enum
 * or counter touched).  cn_predict_orca's humans behave as if the robot were not there; cn_lookahead_actions under
 * CN_HUMANS_ORCA solves ORCA for every one of the K candidates.  In between: the humans react to ONE robot trajectory the
 * caller names — the plan's mean, say — and the table is made once per planning step.
 *   cn_predict_orca_robot writes slot `mode` of cn_predict_orca's table, from the engine's state as it stands, the humans
 *   stepped n_steps times exactly as cn_step steps them on a CN_ROBOT_EXTERNAL engine with robot_visible = 1 and freshly made
 *   simulators (cn_drop_sims) whose robot takes row t of robot_actions at step t.  Row (b, t) is the two doubles at
 *   robot_actions + 2 (b env_stride + t); env_stride counts rows between envs, 0 means n_steps (a dense [B][n_steps][2]
 *   table).  With env_stride = K n, plan->candidates is candidate 0 of every env — the plan's mean under the draw's clip rule.
 * Order of events within step t, CrowdSim.step's: (1) every human solves ORCA against the other humans and the robot WHERE IT
 * STANDS and WITH THE VELOCITY IT HAS (the observation is built before the robot moves; the robot's radius in a human's
 * simulator is float32(radius + 0.01 + human_safety), as any other agent's); (2) the humans move by p + v dt and row t is
 * stored; (3) the robot takes row t: holonomic (vx, vy), used as given and NOT clipped (as cn_rollout_actions and
 * cn_lookahead_actions take theirs), p + v dt; on a CN_UNICYCLE engine ActionRot(v, r): the end point px + cos(theta + r) v dt,
 * theta <- (theta + r) mod 2 pi with python's %, the velocity v (cos, sin)(theta).  The robot starts from the engine's state —
 * position, velocity, radius, cn_get_theta's heading.  It has no swept test, reward, done or time: all n_steps rows are
 * followed and written, as the environment's humans keep stepping behind a `done`.  So for the sequence itself
 * cn_lookahead_paths on this table is cn_lookahead_actions under CN_HUMANS_ORCA on a robot_visible = 1 engine with fresh
 * simulators, bit for bit; for any other candidate scored against it the humans avoid the nominal robot, not that candidate.
 * ANY engine is served — CN_ROBOT_ORCA (its rows are (vx, vy)), CN_UNICYCLE and robot_visible = 0 ones: the humans of THIS
 * call see the robot all the same (nothing of the workgroup is sized by the engine's setting).  ONE launch on the engine's
 * stream, NOT counted in cn_launch_counts; nothing of the engine is written.  Refused, in this order, before anything is
 * enqueued: NULL human_vel: CN_ERR_INVALID; NULL robot_actions: CN_ERR_INVALID naming it; env_stride < 0 or 0 < env_stride <
 * n_steps: CN_ERR_INVALID with both numbers; then cn_predict_orca's refusals, in its order, under this call's name.
 * n_steps == 0: CN_OK, nothing launched, nothing written.  Asynchronous: both arrays must stay valid until the launch has run.
 * Out of scope: clipping or validating the rows; re-predicting between the iterations of one planning step. */
int cn_predict_orca_robot(cn_engine* e, int n_steps, int n_modes, int mode,
                          const double* robot_actions /* DEVICE; row (b, t) at robot_actions + 2 (b env_stride + t) */,
                          int64_t env_stride          /* rows between envs; 0 means n_steps */,
                          double* human_vel           /* DEVICE [B][n_modes][n_steps][A-1][2], 16-byte aligned */);
/* cn_plan_*_predict_orca_rollout with slot orca_mode made by cn_predict_orca_robot on the plan's nominal sequence.  Per real
 * step s, with c = counter + s * iterations:
 *   cn_predict(..); cn_plan_draw(e, cfg, plan, c);
 *   cn_predict_orca_robot(e, cfg->n_steps, M, orca_mode, plan->candidates, K n, pred->human_vel)
 *       — candidates[b][0] of that draw: the mean as it stands after the previous step's shift, under the draw's clip rule;
 *   the paths (M == 1) or modes planner with counter c — its iteration 0 draws with c again, the same bits, so the call does
 *   not launch that draw a second time; cn_rollout_step; cn_plan_shift.
 * ONE prediction per planning step, not one per CEM / MPPI iteration.  Arguments, checks and their order: those of the
 * cn_plan_*_predict_orca_rollout calls, under these names; CN_ROBOT_ORCA engines, and CN_UNICYCLE ones without
 * cn_plan_set_unicycle, stay refused. */
int cn_plan_cem_predict_orca_nominal_rollout (cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                              const cn_plan* plan, const cn_predictors* pred, int orca_mode, uint32_t counter);
int cn_plan_mppi_predict_orca_nominal_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                              const cn_plan* plan, const cn_predictors* pred, int orca_mode, double temperature,
                                              int fit_std, uint32_t counter);

/* ------------------------------------------------------------------------------------------------------
 * The ORCA predictor on hypothesised human goals: M futures in one launch (no version bump: new symbols only; no existing
 * struct, enum, counter or refusal touched).  cn_predict_orca reads every human's goal from the engine's state — the simulator
 * knows it, a planner outside one does not.  Here the goals are an argument, M sets of them per env, and a second call samples
 * such sets from what can be observed.
 *   cn_predict_orca_goals writes cn_predict_orca's table for every mode m of human_vel [B][n_modes][n_steps][A - 1][2] in one
 *   launch: in mode m human h + 1 of env b heads for goals[b][m][h] (two doubles) instead of its goal in the engine's state.
 * Everything else is the engine's as it stands — position, velocity, radius, v_pref, ORCA parameters, max_neighbors, time_step —
 * and everything cn_predict_orca says of its table holds per mode: the robot unseen, fresh simulators, the kd order carried
 * inside the kernel, p + v dt in float64, all n_steps rows always written.  With goals[b][m] the engine's own, mode m is
 * cn_predict_orca's table bit for bit; a mode's rows depend on neither the other modes, M nor B.  A parked placeholder of the
 * `mixed` rule ignores its row of goals and gets what cn_predict_orca gives it.  ANY engine is served.  ONE launch on the
 * engine's stream — step_kernel's workgroup per E of the B M virtual envs (b, m), the engine's LDS per workgroup — NOT counted in
 * cn_launch_counts; nothing of the engine is written (state, cn_rollout_io arrays, ring levels, kd rows, the robot's captured
 * simulator, settings), `goals` is only read.  Refused, in this order, before anything is enqueued: NULL goals, NULL
 * human_vel: CN_ERR_INVALID naming it; n_modes < 1: CN_ERR_INVALID, n_modes > 8: CN_ERR_UNSUPPORTED with the number;
 * n_steps < 0: CN_ERR_INVALID; NULL engine: CN_ERR_INVALID; B n_modes virtual envs or B n_modes n_steps (A - 1) rows beyond an
 * int: CN_ERR_UNSUPPORTED.  n_steps == 0: CN_OK, nothing launched, nothing written.  Asynchronous: both arrays must stay valid
 * until the launch has run.  Out of scope: the robot in sight on hypothesised goals, a per-mode v_pref, a one-call rollout form
 * (the per-step calls are asynchronous already). */
int cn_predict_orca_goals(cn_engine* e, int n_steps, int n_modes,
                          const double* goals /* DEVICE [B][n_modes][A-1][2], 16-byte aligned */,
                          double* human_vel   /* DEVICE [B][n_modes][n_steps][A-1][2], 16-byte aligned */);
/* cn_goal_hypotheses makes such a table of goals on the device, from the engine's state as it stands: one streaming launch, a
 * lane and one 16-byte store per (b, m, h), nothing of the engine written, NOT counted in cn_launch_counts.  Float64, every
 * product, quotient and sum an operation of its own in the order written here.  With (p, v, g) position, velocity and goal of
 * human h + 1 of env b, its nominal offset d is
 *   CN_GOALS_ENGINE   d = (gx - px, gy - py)                                    — the simulator's knowledge, perturbed
 *   CN_GOALS_HEADING  speed = sqrt(vx vx + vy vy); speed > 0: d = ((vx / speed) reach, (vy / speed) reach), else d = (0, 0)
 *                     — `reach` metres along the way it is walking; a standing human is predicted to stay.  g is not read.
 * Mode 0 when nominal_first != 0: ENGINE: g, bit for bit; HEADING: (px + dx, py + dy).  Every other mode: the Philox4x32-10 block
 * of counter words (h, m, b, counter) under key (seed low, seed high) gives u1, u2 and the Box-Muller pair
 * (z1, z2) = (r cos(a), r sin(a)), r = sqrt(-2 log(u1)), a = 2 pi u2, by cn_plan_draw's expressions; then
 *   rot = std_heading z1;  scale = 1 + std_distance z2, 0 where that is negative;  c = cos(rot), s = sin(rot)
 *   goals[b][m][h] = (px + scale (c dx - s dy), py + scale (s dx + c dy)).
 * So a row depends on neither B, M nor A, the same arguments give the same bits, and with both deviations 0 every mode is
 * p + d exactly.  The parked placeholders of the `mixed` rule keep their own goals (they are at rest at them: d = 0 under
 * either base).  crowdnav_amd/predict.py's goal_hypotheses restates it in numpy; the two differ through the device's log, cos
 * and sin alone.  ANY engine is served.  Refused, in this order, before anything is enqueued: NULL goals: CN_ERR_INVALID;
 * n_modes as above; a base that is neither value: CN_ERR_INVALID naming it; reach not finite or not > 0 (read, and checked,
 * under CN_GOALS_HEADING only), std_heading or std_distance not finite or negative: CN_ERR_INVALID naming it; NULL engine:
 * CN_ERR_INVALID.  Asynchronous: goals must stay valid until the launch has run.  Out of scope: inferring goals from a track's
 * history. */
enum { CN_GOALS_ENGINE = 0, CN_GOALS_HEADING = 1 };
int cn_goal_hypotheses(cn_engine* e, int n_modes, int base, double reach, double std_heading, double std_distance,
                       int nominal_first, uint64_t seed, uint32_t counter,
                       double* goals /* DEVICE [B][n_modes][A-1][2], 16-byte aligned */);

#ifdef __cplusplus
}
#endif
#endif /* CROWDNAV_AMD_H */
