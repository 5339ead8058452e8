// Device side of libcrowdnav_amd.so: the batched CrowdSim transition as a wave-level pipeline.
//
// One workgroup = E whole envs (E * A <= 64 agents) on 1..8 waves.  A transition runs in phases that each use
// the lanes differently (all separated by workgroup barriers, all data exchanged through LDS).  The per-agent
// phases run on wave 0 only; the per-pair phases are spread over every wave of the workgroup, and the waves that
// have nothing to do in a phase sleep at the barrier without taking issue slots from other workgroups:
//   stage      lane = agent            float32 view of the agents as rvo2 is told them (orca.py:100-110)
//   pairs-1    lane = (agent, cand.)   squared distance of every ordered pair            (Appendix A.2)
//   pairs-2    lane = (agent, cand.)   stable rank among the agent's candidates -> neighbour slot; the
//                                      ORCA half-plane of that pair -> LDS float4 slot   (Appendix A.3)
//   solve      lane = agent            half-planes -> VGPRs, unrolled 2-D program, rare 3-D fallback
//   collide    lane = human            float64 swept robot-human distance (crowd_sim.py:331-351)
//   reduce     lane = robot            reward / done / info (crowd_sim.py:364-389)
//   integrate  lane = agent            Agent.step (agent.py:127-135)
// The chip is issue/latency-bound on this path (4096 envs x 6 agents = 24.6 k agents on 1024 SIMDs): E and the
// workgroup size are tuning knobs chosen on the host (crowdnav_amd.hip: pick_geometry).
#pragma once
#include <hip/hip_runtime.h>
#include <limits>

#include "../../include/crowdnav_amd.h"
#include "orca_device.h"
#include "kd_order.h"
#include "scenario_device.h"
#include "scenario_wave.h"
#include "transition.h"

namespace cn {

// How the 10-half-plane kernels (crowds of 6+ humans) solve an agent's ORCA program — what was measured on the way is
// profiles/HISTORY.md: the planar program runs on three lanes per agent (orca_device.h: lp_planar_tri), RVO2's 3-D fallback for
// the infeasible agents as lp_relaxed_lazy (one-wave workgroups with room for its candidate rows in d2) or lp_relaxed_coop
// (several waves per workgroup, tiny crowds).  The 5-half-plane kernels solve in candidate form (lp_line_candidate /
// lp_planar_scan, lp3_project / lp3_scan).

constexpr int kMaxBlock = 512;  // threads per workgroup of the transition kernels (1..8 waves)

struct Params {
    int B, A;          // envs, agents per env
    int E;             // envs per workgroup (their E * A agents are lanes of wave 0)
    int threads;       // workgroup size (= blockDim.x of the transition kernels; read from HERE in the step loop: blockDim.x
                       // is a load from the dispatch packet — a global load and a wait per use): wave 0 runs the per-agent
                       // phases, every wave the per-pair phases
    int nA;            // E * A agent lanes
    int NC;            // A - 1 candidate neighbours per agent
    int pairs;         // nA * NC
    int ring_depth;    // D: scenarios a launch may look ahead of an env's next one
    int robot_visible, robot_orca;
    int robot_unicycle;  // external robot actions are ActionRot(v, r) (agent.py:115-135)
    int async_fill;      // CN_FLAG_ASYNC_SCENARIO_FILL: ring slots are published one by one (StateView::ring_ready)
    int sched;           // the 20-human shard's kernel: sub-launch 0..3 of the 3-of-4 env schedule (launch_shard), -1 = all envs,
                         // kSchedDynamic = persistent workgroups taking (env, visit) items from a device queue
    int dyn_visits;      // ... visits per env and call under the dynamic schedule (launch_shard: ~56 steps per visit)
    int kd;              // A > 10: some rvo2 simulator of an env holds more than 10 agents and splits its kd-tree (kd_order.h)
    KdLayout kdl;        // ... and where its bookkeeping lives in LDS (offsets from Smem::kd_off)
    double dt, time_limit, success_reward, collision_penalty, discomfort_dist, discomfort_factor;
    double robot_safety, human_safety;
    OrcaParams orca;
    int ring_mod;      // C: ring slots per env, ordinal o lives in slot o % C (D, or 2 D with the lagged fill: fill_plan.h); last,
                       // so that every other field keeps its place in the kernels' argument blocks
};

struct StateView {
    double2* pos;
    double2* vel;
    double2* goal;
    double2* rv;  // (radius, v_pref)
    double* gtime;
    double* theta;          // [B] robot heading (only a unicycle robot changes it)
    float* rsim_radius;     // [B*A] radii captured by the robot's persistent ORCA policy (orca.py:98-104)
    float* rsim_max_speed;  // [B]
    uint8_t* rsim_valid;    // [B]
    uint32_t* mt_key;       // [624][B]   generator state of the env's own stream
    uint32_t* ring_mt_key;  // [624][kRedoLanes] HBM generator scratch of ring_redo_kernel (scenarios the head generator gave up on)
    int2* redo_list;        // [B*C] (ring index, seed) of those scenarios; redo_count [0] = how many (zeroed before a fill)
    int* redo_count;        // [2] ... and [1] = entries of first_list (below), zeroed with it
    int* mt_pos;            // [B]
    // scenario ring: the next ring_depth episodes of every env, generated ahead of the rollout
    double2* ring_pos;      // [B][C][A]
    double2* ring_goal;
    double2* ring_rv;
    int* ring_filled_in;    // [B] episode ordinals < this have been generated (read side)
    int* ring_filled_out;   // [B] (written by the fill kernel; the host swaps the two)
    int* ring_ready;        // [B*D] async fill: ordinal + 1 of the scenario a slot holds, stored with release once it is complete
    int* ring_claim;        // [B*D] async fill: ordinal + 1 some fill launch is generating (or has generated) for the slot
    uint8_t* kd_order;      // [B*A][kd_row_bytes(A)] the permutation each agent's rvo2 simulator partitions in place (kd_order.h)
    uint8_t* kd_valid;      // [B*A] 0 = a freshly built simulator (identity order)
    // scenario cache of the wave generators (cached_scenario): a rollout whose episode seeds come from a SMALL set (seed_mod <=
    // kScenarioCacheMax: the reference's 'val' / 'test' phases replay 100 / 500 fixed cases) generates every scenario once
    double2* cache_pos;     // [kScenarioCacheMax][A]
    double2* cache_goal;
    double2* cache_rv;
    int* cache_state;       // [kScenarioCacheMax] 0 = empty, 1 = complete (release / acquire at agent scope)
    int cache_n;            // seeds cached by the current rollout (io.seed_mod), 0 = off
    int* error;             // [1] the engine's error word (ScenarioCfg::error): bit 2 = a visit of the dynamic schedule gave up waiting
    int* dyn_queue;         // [1 + B] dynamic schedule of the shard kernel: [0] next (env, visit) item, [1 + env] visits env has COMPLETED
    int* ep_word;           // [B] (episodes finished << 2) | io.active state, ONE word stored by the rollout kernels next to the
                            // two io arrays: the asynchronous fill reads it for a consistent (state, ep_count) snapshot
    // launch epilogue of the rollout kernels (rollout_epilogue): arrival tickets and partial sums
    double* wg_partial;     // [workgroups][CN_SUMMARY_FIELDS + 1] per-workgroup sums over its envs' record rings, its transitions
    double* group_partial;  // [kEpilogueGroups][CN_SUMMARY_FIELDS + 1]
    unsigned* tickets;      // [(kEpilogueGroups + 1) * kTicketStride] arrivals per group, then of the group leaders, one
                            // counter per 256-byte line; zero between launches
    // First step of every ring scenario, solved when its slot is filled (rollout_fused.h: ring_first_step_kernel) for the engines
    // whose cn_rollout runs the two-wave kernel; 1-element placeholders elsewhere.  Last, so that every field above keeps its offset.
    float2* ring_vel0;          // [B][C][A] the velocity every agent's ORCA solve yields for the scenario's first step
    uint8_t* ring_vel0_ok;      // [B*C] 1: ring_vel0 of the slot belongs to the scenario it holds and to the robot's simulator as it is
    int* first_list;            // [B*C] ring indices a fill generated into (ring_fill_kernel); how many: redo_count[1]
    unsigned int* fresh_counts; // [2] two-wave kernel: episode starts that adopted ring_vel0; iterations redone (cn_fresh_starts)
};

constexpr int kEpilogueGroups = 32;  // workgroup b arrives at counter b % 32: 64 arrivals per counter at 2048 workgroups
constexpr int kTicketStride = 64;    // counters 256 bytes apart: same-line atomics serialise at ~10 ns each

struct StepIo {
    const double* action;
    double* reward;
    uint8_t* done;
    uint8_t* info;
    double* dmin;
    double* action_out;
    float* orca_vel;
    double* obs;
    int update;
};

// ---------------------------------------------------------------------------------------------- LDS carve-up
struct Smem {
    float4* kin;      // [nA + 1] float32(px, py, vx, vy); slot nA = (+inf, +inf, 0, 0): the "candidate" of a pair that does not exist
    double2* posd;    // [nA] float64 position
    double2* act;     // [nA] (robot lanes) applied robot action
    float4* lines;    // [nA][kLineStride] ORCA half-planes, slot = neighbour rank
    float4* proj;     // [nA][kLineStride] projected half-planes (3-D fallback scratch)
    float4* cand2;    // [nA][kLineStride] candidate form: 1-D solutions of the agent's half-planes (lp_line_candidate)
    float4* cand3;    // [nA][kLineStride] ... and of its projected half-planes (3-D fallback)
    double* rad;      // [nA] float64 radius
    double* closest;  // [nA] (human lanes) closest boundary distance during the step
    float* hview;     // [nA] radius as a human's rvo2 sim holds it: float32(radius + 0.01 + human_safety)
    float* rview;     // [nA] radius as the robot's rvo2 sim holds it (captured, see load_robot_view)
    float* d2;        // [pairs] squared distance agent -> candidate (+inf if the pair does not exist)
    int* pinfo;       // [pairs] packed pair descriptor
    int* count;       // [nA] neighbours kept
    int* flag;        // [nA] (robot lanes) per-env flag broadcast
    float4* sol;      // [nA] lane-cooperative program input: (pref.x, pref.y, maxSpeed, solve ? 1 : 0)
    float4* res;      // [nA] ... and output: (result.x, result.y, first infeasible line or n, -)
    int* todo;        // [nA + 1] agents that need the 3-D fallback, compacted; [nA] = how many
    double* disc;     // [kMaxDiscount] discount table gamma^(t dt v_pref) (rollout kernel only)
    uint32_t kd_off;  // byte offset (from the start of LDS) of the kd-tree region, simulators of more than 10 agents: kd_view
    double2* goal2;   // [nA] COMPACT only: the agent's goal ...
    double* vpref;    // [nA] ... and preferred speed: per-episode constants the step loop does not hold in registers
};

constexpr int kCompactScratchDoubles = 16;  // COMPACT: Smem::disc holds the step parameters and the robot lane's bookkeeping instead
constexpr int kMaxDiscount = 256;  // steps per episode the LDS copy of the discount table covers
__host__ __device__ inline size_t proj_bytes(int nA, int /*maxl*/) { return (size_t)16 * kLineStride * nA; }

// maxl: the 5-half-plane kernels have two candidate-form buffers (cand2, cand3); the 10-half-plane kernels none (their lazy
// fallback's candidate rows live in d2)
__host__ __device__ inline size_t smem_bytes(int nA, int pairs, int maxl, int A = 0, int E = 1) {
    return (size_t)nA * (16 + 16 + 16 + (maxl == 5 ? 3 : 1) * 16 * kLineStride + 16 + 16 + 8 + 8 + 4 + 4 + 4 + 4 + 4) + proj_bytes(nA, maxl) +
           (size_t)pairs * 8 + 64 + 8 + 16 + 16 + sizeof(double) * kMaxDiscount + (A > kKdLeaf ? 16 + kd_lds_bytes(nA, A, E) : 0);
}

// COMPACT: the LDS layout of the 20-human shard's kernel (rollout_kernel<10, false, true, true>: one env per one-wave
// workgroup, lazy fallback, two-sweep pair phase).  18.6 KB per workgroup allowed 8 workgroups = 2 waves per SIMD whatever the
// register count; a third resident wave needs <= 12.8 KB (160 KB in 1280-byte granules: 10 granules x 12 workgroups).  What goes:
//   disc   2048 B  the discount table: one global load per step on the robot lane, issued a step ahead of its use
//   proj   3696 -> 1008 B  rows of the lazy fallback belong to the 7 lane groups of a pass, not to the 21 agents (the `kept`
//                  table of the two-sweep pair phase, 840 B, shares them as before)
//   act     336 -> 16 B    one robot per workgroup
//   pinfo  1680 -> 840 B   16-bit pair descriptors (the candidate slot is p - 20 q)
//   kd visit order + traversal stacks  1008 -> 0 B   needed only while exact distance ties are resolved, when `lines` holds
//                  nothing that is not recomputed afterwards (kd_resolve_ties re-runs the half-plane sweep): kd_scratch_view
// and what comes in: the step parameters, the robot lane's episode bookkeeping (128 B), the agents' goals and preferred
// speeds (504 B) — values the step loop would otherwise hold in VGPRs across every phase (third resident wave per SIMD).
constexpr int kLazyRows = (kWave / (kMaxNb - 1)) * (kMaxNb - 1);  // 63 float4: 7 groups x 9 projected half-planes
__host__ __device__ inline size_t smem_bytes_compact(int nA, int pairs, int A, int E) {
    size_t n = (size_t)16 * (nA + 1) + 16 * nA + 16 * E + (size_t)16 * kLineStride * nA + 16 * kLazyRows;
    n += (size_t)nA * (16 + 16 + 16 + 8 + 8 + 8 + 4 + 4 + 4 + 4) + 4 * (nA + 1) + 16;
    n += (size_t)pairs * 4 + (size_t)pairs * 2 + 16 + 16 + 8 * kCompactScratchDoubles + (A > kKdLeaf ? 16 + kd_lds_bytes(nA, A, E) : 0);
    // the traversal scratch of the tie resolver (visit order + stacks, the LAST two arrays of the kd region) lives in `lines`
    if (A > kKdLeaf) n -= (size_t)nA * kd_row_bytes(A) + (size_t)nA * (kd_max_nodes(A) + 1) * 2;
    return n;
}

template <int MAXL, bool COMPACT = false>
__device__ __forceinline__ Smem carve(const Params& P) {
    extern __shared__ double2 smem_raw[];
    Smem s;
    char* p = reinterpret_cast<char*>(smem_raw);
    const int nA = P.nA;
    s.kin = reinterpret_cast<float4*>(p), p += 16 * (nA + 1);
    s.posd = reinterpret_cast<double2*>(p), p += 16 * nA;
    s.act = reinterpret_cast<double2*>(p), p += 16 * (COMPACT ? P.E : nA);
    s.lines = reinterpret_cast<float4*>(p), p += 16 * kLineStride * nA;
    s.proj = reinterpret_cast<float4*>(p), p += COMPACT ? (size_t)16 * kLazyRows : proj_bytes(nA, MAXL);
    s.cand2 = s.cand3 = nullptr;
    if (MAXL == 5) {
        s.cand2 = reinterpret_cast<float4*>(p), p += 16 * kLineStride * nA;
        s.cand3 = reinterpret_cast<float4*>(p), p += 16 * kLineStride * nA;
    }
    s.sol = reinterpret_cast<float4*>(p), p += 16 * nA;
    s.res = reinterpret_cast<float4*>(p), p += 16 * nA;
    s.goal2 = nullptr, s.vpref = nullptr;
    if (COMPACT) {
        s.goal2 = reinterpret_cast<double2*>(p), p += 16 * nA;
        s.vpref = reinterpret_cast<double*>(p), p += 8 * nA;
    }
    s.rad = reinterpret_cast<double*>(p), p += 8 * nA;
    s.closest = reinterpret_cast<double*>(p), p += 8 * nA;
    s.hview = reinterpret_cast<float*>(p), p += 4 * nA;
    s.rview = reinterpret_cast<float*>(p), p += 4 * nA;
    s.count = reinterpret_cast<int*>(p), p += 4 * nA;
    s.flag = reinterpret_cast<int*>(p), p += 4 * nA;
    s.todo = reinterpret_cast<int*>(p), p += 4 * (nA + 1);
    p += (16 - (reinterpret_cast<size_t>(p) & 15)) & 15;  // rows of d2 are read as float4 when NC is a multiple of 4
    s.d2 = reinterpret_cast<float*>(p), p += 4 * P.pairs;
    s.pinfo = reinterpret_cast<int*>(p), p += (COMPACT ? 2 : 4) * P.pairs;
    s.disc = reinterpret_cast<double*>(p + ((8 - (reinterpret_cast<size_t>(p) & 7)) & 7));
    {
        char* q = reinterpret_cast<char*>(s.disc + (COMPACT ? kCompactScratchDoubles : kMaxDiscount));
        q += (16 - (reinterpret_cast<size_t>(q) & 15)) & 15;
        s.kd_off = (uint32_t)(q - reinterpret_cast<char*>(smem_raw));
    }
    return s;
}

// COMPACT (the 20-human shard's kernel): the seven float64 parameters of a step are not held in registers across the step
// loop (14 VGPRs) but kept in LDS — Smem::disc[0..6], written once per launch — and requested where a phase needs them;
// Smem::disc[8..14] hold the robot lane's episode bookkeeping between steps (EpisodeLds, further down).
enum { kParDt = 0, kParLimit, kParSuccess, kParCollision, kParDDist, kParDFactor, kParHSafety, kParCount };
template <bool COMPACT>
__device__ __forceinline__ double step_param(const Params& P, const Smem& s, int which) {
    if (COMPACT) return s.disc[which];
    return which == kParDt ? P.dt : which == kParLimit ? P.time_limit : which == kParSuccess ? P.success_reward :
           which == kParCollision ? P.collision_penalty : which == kParDDist ? P.discomfort_dist :
           which == kParDFactor ? P.discomfort_factor : P.human_safety;
}

// Workgroup barrier of the step / rollout kernels.  A workgroup of ONE wave (P.threads == 64: a compile-time fact in the
// 20-human shard's instantiation, a uniform branch elsewhere) needs no s_barrier: a wave's LDS instructions execute in order,
// so between one lane's write and another lane's read only the compiler has to keep program order — and the s_waitcnt
// lgkmcnt(0) in front of every s_barrier (the LDS queue drained a dozen times per step) goes away.
__device__ __forceinline__ void block_sync(const Params& P) {
    if (P.threads == kWave) wave_lds_sync();
    else __syncthreads();
}
__device__ __forceinline__ int block_sync_or(const Params& P, int v) {
    if (P.threads == kWave) return __ballot(v != 0) != 0ull ? 1 : 0;
    return __syncthreads_or(v);
}

// ---------------------------------------------------------------------------------------------- lanes
struct Lane {
    int lane, env, a, ebase;  // ebase = lane of this env's robot
    bool valid;               // this lane owns an agent of an existing env
    size_t gi;                // env * A + a
};

__device__ __forceinline__ Lane lane_of(const Params& P, int block = -1, int tid = -1) {
    Lane L;
    L.lane = tid < 0 ? (int)threadIdx.x : tid;
    const int el = L.lane / P.A;
    L.a = L.lane - el * P.A;
    L.env = (block < 0 ? (int)blockIdx.x : block) * P.E + el;
    L.valid = (L.lane < P.nA) && (L.env < P.B);
    L.ebase = el * P.A;
    L.gi = (size_t)L.env * P.A + L.a;
    return L;
}

struct AgentRegs {
    double px, py, vx, vy, gx, gy, rad, vpref;
};

__device__ __forceinline__ void load_agent(const StateView& S, size_t gi, AgentRegs& r) {
    const double2 p = S.pos[gi], v = S.vel[gi], g = S.goal[gi], q = S.rv[gi];
    r.px = p.x, r.py = p.y, r.vx = v.x, r.vy = v.y, r.gx = g.x, r.gy = g.y, r.rad = q.x, r.vpref = q.y;
}

// Pair descriptors (agent lane q, candidate slot c): built once per launch.  Candidate order = the order
// ORCA.predict adds the others to its rvo2 sim: the other humans by index, then the robot if it is visible
// (crowd_sim.py:325-327, orca.py:102-104); the robot's own sim holds every human.
//   bits 0-7 agent lane, 8-15 lane of the candidate, 16-23 candidate slot, 24 pair exists, 25 agent is a robot
// COMPACT: 16 bits per pair — bits 0-4 agent lane, 5-9 lane of the candidate, 10 pair exists, 11 agent is a robot; the
// candidate slot is p - NC * agent lane.  pair_info() hands out the 32-bit form either way.
template <bool COMPACT>
__device__ __forceinline__ int pair_info(const Params& P, const Smem& s, int p) {
    if (!COMPACT) return s.pinfo[p];
    const int w = reinterpret_cast<const uint16_t*>(s.pinfo)[p];
    const int q = w & 31;
    return q | (((w >> 5) & 31) << 8) | ((p - q * P.NC) << 16) | (((w >> 10) & 3) << 24);
}

template <bool COMPACT = false>
__device__ __forceinline__ void build_pairs(const Params& P, const Smem& s, bool every_env_exists = false) {
    for (int p = threadIdx.x; p < P.pairs; p += P.threads) {
        const int q = p / P.NC;
        const int c = p - q * P.NC;
        const int el = q / P.A;
        const int a = q - el * P.A;
        int j;
        bool exists = every_env_exists || ((int)blockIdx.x * P.E + el) < P.B;
        if (a == 0) {
            j = c + 1;
        } else {
            j = c + 1 + (c + 1 >= a ? 1 : 0);
            if (j >= P.A) {
                j = 0;
                exists = exists && P.robot_visible;
            }
        }
        if (COMPACT)
            reinterpret_cast<uint16_t*>(s.pinfo)[p] = (uint16_t)(q | ((el * P.A + j) << 5) | (exists ? 1 << 10 : 0) | (a == 0 ? 1 << 11 : 0));
        else
            s.pinfo[p] = q | ((el * P.A + j) << 8) | (c << 16) | (exists ? 1 << 24 : 0) | (a == 0 ? 1 << 25 : 0);
    }
}

// The robot's ORCA policy object outlives episodes and keeps the radii / max speed it saw when its rvo2
// simulator was first built (orca.py:95-104).  Load or capture them.
//   preloaded: the caller requested rsim_valid / rsim_radius / rsim_max_speed earlier (sarl_decide_step_kernel, at its top)
__device__ __forceinline__ void load_robot_view(const Params& P, const StateView& S, const Smem& s,
                                                const Lane& L, const AgentRegs& r, float& robot_max_speed, bool preloaded = false,
                                                bool pre_have = false, float pre_radius = 0.0f, float pre_max_speed = 0.0f) {
    robot_max_speed = 0.0f;
    if (!L.valid) return;
    const bool have = preloaded ? pre_have : S.rsim_valid[L.env] != 0;
    float rr;
    if (have) {
        rr = preloaded ? pre_radius : S.rsim_radius[L.gi];
    } else {
        rr = (float)(r.rad + 0.01 + P.robot_safety);
        S.rsim_radius[L.gi] = rr;
    }
    s.rview[L.lane] = rr;
    if (L.a == 0) {
        if (have) {
            robot_max_speed = preloaded ? pre_max_speed : S.rsim_max_speed[L.env];
        } else {
            robot_max_speed = (float)r.vpref;
            S.rsim_max_speed[L.env] = robot_max_speed;
        }
    }
}

// ---------------------------------------------------------------------------------------------- kd-tree order (kd_order.h)
// The kd region's pointers: region offset + the host-computed layout in the kernel arguments (KdLayout).
__device__ __forceinline__ KdSmem kd_view(const Params& P, const Smem& s) {
    extern __shared__ double2 smem_raw[];
    return kd_carve(reinterpret_cast<char*>(smem_raw) + s.kd_off, P.kdl);
}

// COMPACT: the tie resolver's traversal scratch is carved out of `lines` (see carve)
template <bool COMPACT>
__device__ __forceinline__ KdSmem kd_scratch_view(const Params& P, const Smem& s) {
    KdSmem k = kd_view(P, s);
    if (COMPACT) {
        k.visit = reinterpret_cast<uint8_t*>(s.lines);
        k.stack = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(s.lines) + (size_t)P.nA * k.row);
    }
    return k;
}

// A launch keeps the permutations of its envs' simulators in LDS: loaded here (or built fresh), stored by kd_store.
__device__ __forceinline__ void kd_load(const Params& P, const StateView& S, const Smem& s, const Lane& L) {
    if (!P.kd) return;
    const KdSmem k = kd_view(P, s);
    if (L.lane < P.nA) {
        uint8_t* row = k.ord + (size_t)L.lane * k.row;
        if (L.valid && S.kd_valid[L.gi] != 0) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(S.kd_order + L.gi * k.row);
            for (int w = 0; w < k.row / 4; ++w) reinterpret_cast<uint32_t*>(row)[w] = src[w];
        } else {
            kd_identity_row(row, k.row, P.A, L.a, P.robot_visible);
        }
    }
    if (threadIdx.x == 0) *k.gen = 0;
    for (int i = threadIdx.x; i < P.E * 2 * 2; i += P.threads) k.count[i] = 0;  // no "last step's tree" yet
}

__device__ __forceinline__ void kd_store(const Params& P, const StateView& S, const Smem& s, const Lane& L) {
    if (!P.kd || !L.valid) return;
    const KdSmem k = kd_view(P, s);
    const uint32_t* row = reinterpret_cast<const uint32_t*>(k.ord + (size_t)L.lane * k.row);
    uint32_t* dst = reinterpret_cast<uint32_t*>(S.kd_order + L.gi * k.row);
    for (int w = 0; w < k.row / 4; ++w) dst[w] = row[w];
    S.kd_valid[L.gi] = 1;
}

// A new episode: every Human is rebuilt and with it its ORCA policy and simulator (crowd_sim.py:155-207); the robot's
// policy object, hence its simulator, lives on.  Called by the lanes of an env that has just loaded its next scenario.
__device__ __forceinline__ void kd_new_episode(const Params& P, const Smem& s, const Lane& L) {
    if (!P.kd) return;
    const KdSmem k = kd_view(P, s);
    if (L.a > 0) kd_identity_row(k.ord + (size_t)L.lane * k.row, k.row, P.A, L.a, P.robot_visible);
    if (L.a == 0) {  // nothing of this env's last tree says anything about the fresh rows
        const int last = *k.gen, el = L.ebase / P.A;
        k.count[(last * P.E + el) * 2 + 0] = 0;
        k.count[(last * P.E + el) * 2 + 1] = 0;
    }
}

// The tree(s) of every env of the workgroup from this step's float32 positions (s.kin), breadth first on agent sets: the
// nodes that split, in `generation` g of the node lists.  All threads (barriers inside).
__device__ __forceinline__ void kd_build_trees(const Params& P, const Smem& s, const Lane& L, int g) {
    const KdSmem k = kd_view(P, s);
    const int tid = threadIdx.x;
    const bool agent = L.lane < P.nA;
    const int el = agent ? L.ebase / P.A : 0;
    const float4 me = agent ? s.kin[L.lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t kx = kd_key(me.x), ky = kd_key(me.y);
    const uint64_t amask = P.A >= 64 ? ~0ull : ((1ull << P.A) - 1ull);
    for (int t = 0; t < 2; ++t) {
        KdNode* list = k.nodes + ((size_t)(g * P.E + el) * 2 + t) * k.mn;
        int* cnt = k.count + (g * P.E + el) * 2 + t;
        if (!kd_tree_on(P.A, t, P.robot_visible)) {  // uniform
            if (agent && L.a == 0) *cnt = 0;
            continue;
        }
        for (int i = tid; i < P.E * k.mn; i += P.threads) {
            k.bb[4 * i + 0] = 0xffffffffu, k.bb[4 * i + 1] = 0u, k.bb[4 * i + 2] = 0xffffffffu, k.bb[4 * i + 3] = 0u;
        }
        const KdNode* old = k.nodes + ((size_t)((g ^ 1) * P.E + el) * 2 + t) * k.mn;
        const int n_old = agent ? k.count[((g ^ 1) * P.E + el) * 2 + t] : 0;
        int first_dirty = 1 << 20;
        if (agent && L.a == 0) {  // the env's robot lane keeps the books (whether or not the robot is in this tree)
            list[0].meta = (uint32_t)kd_tree_size(P.A, t) << 8;
            list[0].set = t == 0 ? amask : (amask & ~1ull);
            *cnt = 1;
        }
        block_sync(P);
        for (int r = 0;; ++r) {
            const int c = agent ? *cnt : 0;
            const bool live = agent && r < c;
            if (!block_sync_or(P, live ? 1 : 0)) break;
            KdNode nd = KdNode{0u, 0u, 0ull, 0ull, 0ull};
            bool member = false;
            uint32_t* acc = k.bb + ((size_t)el * k.mn + r) * 4;
            if (live) {
                nd = list[r];
                member = (t == 0 || L.a > 0) && ((nd.set >> L.a) & 1ull) != 0ull;
                if (member) {
                    atomicMin(acc + 0, kx), atomicMax(acc + 1, kx);
                    atomicMin(acc + 2, ky), atomicMax(acc + 3, ky);
                }
            }
            block_sync(P);
            bool lower = false;
            if (live) {
                const float min_x = kd_unkey(acc[0]), max_x = kd_unkey(acc[1]), min_y = kd_unkey(acc[2]), max_y = kd_unkey(acc[3]);
                const bool vertical = (max_x - min_x) > (max_y - min_y);
                const float split = vertical ? 0.5f * (max_x + min_x) : 0.5f * (max_y + min_y);
                lower = member && (vertical ? me.x : me.y) < split;
            }
            const unsigned long long ballot = __ballot(lower);
            if (live && L.a == 0) {
                const uint64_t lm = (ballot >> L.ebase) & amask;
                const int begin = nd.meta & 0xff, end = (nd.meta >> 8) & 0xff, nl = __popcll(lm);
                const bool degenerate = nl == 0;
                const uint32_t meta = (uint32_t)begin | ((uint32_t)end << 8) | ((uint32_t)nl << 16) | (degenerate ? 1u << 24 : 0u);
                list[r].meta = meta;
                list[r].left = lm;
                if (first_dirty > r && (r >= n_old || old[r].meta != meta || old[r].left != lm)) first_dirty = r;
                int n = c;
                if (!degenerate && nl > kKdLeaf && n < k.mn) {
                    list[n].meta = (uint32_t)begin | ((uint32_t)(begin + nl) << 8);
                    list[n].set = lm;
                    ++n;
                }
                if (!degenerate && end - begin - nl > kKdLeaf && n < k.mn) {
                    list[n].meta = (uint32_t)(begin + nl) | ((uint32_t)end << 8);
                    list[n].set = nd.set & ~lm;
                    ++n;
                }
                *cnt = n;
                k.dirty[el * 2 + t] = first_dirty;
            }
        }
    }
}

// The same for the usual geometry of these crowds — one env per single-wave workgroup: every quantity of a node is uniform
// over the wave, so the bounding box is four DPP wave reductions, the lower side a ballot, and the control flow scalar: no LDS
// atomics, no barriers (the cooperative version above spent ~1 400 clock ticks per node on them).
// Built every step although 84 % of the steps (20 humans) leave the tree as it was.  Proving "unchanged" first — the four
// agents that attained a node's box last time still bound its members, every member still on its side of the new split: one
// vector pass over (node, agent) lanes, nearly free — was built and measured: the 29 % of steps that then DID rebuild paid
// 12 900 clock ticks each instead of 3 100, because code a wave executes once in a while is not in the instruction cache
// when it comes (the step loop of this kernel is ~45 KB by itself), 3 780 vs 3 100 ticks per step on average.  What the
// builder does hand on is the first node whose record differs from last step's: in unchanged steps the simulator lanes do
// nothing.  Returns the generation that holds this step's lists.
__device__ __forceinline__ int kd_build_trees_wave(const Params& P, const Smem& s, const Lane& L, int g_last) {
    const KdSmem k = kd_view(P, s);
    const bool agent = L.lane < P.nA;  // = L.lane < P.A: one env
    const float4 me = agent ? s.kin[L.lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t kx = kd_key(me.x), ky = kd_key(me.y);
    const uint64_t amask = P.A >= 64 ? ~0ull : ((1ull << P.A) - 1ull);
    const int g = g_last ^ 1;
    for (int t = 0; t < 2; ++t) {
        KdNode* list = k.nodes + ((size_t)g * 2 + t) * k.mn;
        const KdNode* old = k.nodes + ((size_t)g_last * 2 + t) * k.mn;
        int* cnt = k.count + g * 2 + t;
        if (!kd_tree_on(P.A, t, P.robot_visible)) {
            if (L.lane == 0) *cnt = 0, k.dirty[t] = 0;
            continue;
        }
        const int n_old = k.count[g_last * 2 + t];
        int first_dirty = 1 << 20, n = 1;
        if (L.lane == 0) {
            list[0].meta = (uint32_t)kd_tree_size(P.A, t) << 8;
            list[0].set = t == 0 ? amask : (amask & ~1ull);
        }
        for (int r = 0; r < n; ++r) {  // n, r, the node and everything derived from it are wave-uniform
            const KdNode nd = list[r];
            const bool had = r < n_old;
            const KdNode od = old[had ? r : 0];
            const bool member = agent && ((nd.set >> L.lane) & 1ull) != 0ull;
            uint32_t b0 = member ? kx : 0xffffffffu, b1 = member ? kx : 0u, b2 = member ? ky : 0xffffffffu, b3 = member ? ky : 0u;
            kd_wave_bbox(b0, b1, b2, b3);
            const float min_x = kd_unkey(b0), max_x = kd_unkey(b1), min_y = kd_unkey(b2), max_y = kd_unkey(b3);
            const bool vertical = (max_x - min_x) > (max_y - min_y);
            const float split = vertical ? 0.5f * (max_x + min_x) : 0.5f * (max_y + min_y);
            const uint64_t lm = __ballot(member && (vertical ? me.x : me.y) < split) & amask;
            const int begin = nd.meta & 0xff, end = (nd.meta >> 8) & 0xff, nl = __popcll(lm);
            const bool degenerate = nl == 0;
            const uint32_t meta = (uint32_t)begin | ((uint32_t)end << 8) | ((uint32_t)nl << 16) | (degenerate ? 1u << 24 : 0u);
            if (first_dirty > r && (!had || od.meta != meta || od.left != lm)) first_dirty = r;
            const bool lo = !degenerate && nl > kKdLeaf && n < k.mn;
            const bool hi = !degenerate && end - begin - nl > kKdLeaf && n + (lo ? 1 : 0) < k.mn;
            if (L.lane == 0) {
                list[r].meta = meta;
                list[r].left = lm;
                if (lo) {
                    list[n].meta = (uint32_t)begin | ((uint32_t)(begin + nl) << 8);
                    list[n].set = lm;
                }
                if (hi) {
                    list[n + (lo ? 1 : 0)].meta = (uint32_t)(begin + nl) | ((uint32_t)end << 8);
                    list[n + (lo ? 1 : 0)].set = nd.set & ~lm;
                }
            }
            n += (lo ? 1 : 0) + (hi ? 1 : 0);
        }
        if (L.lane == 0) *cnt = n, k.dirty[t] = first_dirty;
    }
    return g;
}

// Every simulator's permutation follows this step's tree (lane = the simulator's own agent).  A node whose record equals
// last step's, under ancestors that did not move anything either, is partitioned already.
__device__ __forceinline__ void kd_update_orders(const Params& P, const Smem& s, const Lane& L, int g) {
    const KdSmem k = kd_view(P, s);
    if (L.lane >= P.nA) return;
    const int el = L.ebase / P.A, t = kd_tree_of(L.a, P.robot_visible);
    if (!kd_tree_on(P.A, t, P.robot_visible)) return;
    const KdNode* cur = k.nodes + ((size_t)(g * P.E + el) * 2 + t) * k.mn;
    const KdNode* old = k.nodes + ((size_t)((g ^ 1) * P.E + el) * 2 + t) * k.mn;
    const int n_cur = k.count[(g * P.E + el) * 2 + t], n_old = k.count[((g ^ 1) * P.E + el) * 2 + t];
    uint8_t* row = k.ord + (size_t)L.lane * k.row;
    (void)old, (void)n_old;
    // every node from the first one whose record differs from last step's (the builder found it): conservative — a later node
    // of another subtree is partitioned already and is left as it is by a second partition
    for (int r = k.dirty[el * 2 + t]; r < n_cur; ++r) {
        const KdNode c = cur[r];
        if (((c.meta >> 24) & 1u) != 0u) continue;
        if (P.A <= 32)
            kd_partition32(row, c.meta & 0xff, (c.meta >> 8) & 0xff, (c.meta >> 16) & 0xff, (uint32_t)c.left);
        else
            kd_partition(row, c.meta & 0xff, (c.meta >> 8) & 0xff, (c.meta >> 16) & 0xff, c.left);
    }
}

// Position of every agent of this lane's simulator in RVO2's traversal of its tree (queryAgentTreeRecursive without the
// pruning, which only drops candidates that would be rejected): nearer child first, a leaf in permutation order.  Serial on
// the lane; runs only for simulators with an exact distance tie.
template <bool COMPACT = false>
__device__ __forceinline__ void kd_visit_order(const Params& P, const Smem& s, const Lane& L, int g) {
    const KdSmem k = kd_scratch_view<COMPACT>(P, s);
    const int el = L.ebase / P.A, t = kd_tree_of(L.a, P.robot_visible);
    const KdNode* cur = k.nodes + ((size_t)(g * P.E + el) * 2 + t) * k.mn;
    const int n_cur = kd_tree_on(P.A, t, P.robot_visible) ? k.count[(g * P.E + el) * 2 + t] : 0;
    const uint8_t* row = k.ord + (size_t)L.lane * k.row;
    uint8_t* vis = k.visit + (size_t)L.lane * k.row;
    uint16_t* st = k.stack + (size_t)L.lane * (k.mn + 1);
    const float4 me = s.kin[L.lane];
    auto box_dist = [&](int b, int e) {
        float4 q = s.kin[L.ebase + row[b]];
        float min_x = q.x, max_x = q.x, min_y = q.y, max_y = q.y;
        for (int p = b + 1; p < e; ++p) {
            q = s.kin[L.ebase + row[p]];
            max_x = fmaxf(max_x, q.x), min_x = fminf(min_x, q.x);
            max_y = fmaxf(max_y, q.y), min_y = fminf(min_y, q.y);
        }
        const float a0 = fmaxf(0.0f, min_x - me.x), a1 = fmaxf(0.0f, me.x - max_x);
        const float a2 = fmaxf(0.0f, min_y - me.y), a3 = fmaxf(0.0f, me.y - max_y);
        return ((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3;
    };
    int sp = 0, next = 0;
    st[sp++] = (uint16_t)(kd_tree_size(P.A, t) << 8);
    while (sp > 0) {
        const int e = st[--sp];
        const int b = e & 0xff, en = e >> 8;
        int nl = 0;
        if (en - b > kKdLeaf)
            for (int r = 0; r < n_cur; ++r) {
                const uint32_t m = cur[r].meta;
                if ((m & 0xffffu) == (uint32_t)e && ((m >> 24) & 1u) == 0u) nl = (m >> 16) & 0xff;
            }
        if (nl > 0) {
            const float dl = box_dist(b, b + nl), dr = box_dist(b + nl, en);
            const uint16_t lo = (uint16_t)(b | ((b + nl) << 8)), hi = (uint16_t)((b + nl) | (en << 8));
            st[sp++] = dl < dr ? hi : lo;  // the farther child waits
            st[sp++] = dl < dr ? lo : hi;
        } else {
            for (int p = b; p < en; ++p) vis[row[p]] = (uint8_t)next++;
        }
    }
}

// Second sweep of the 20-candidate pair phase (orca_phases, two_sweeps): lane = (agent, slot), 6 agents per pass of a wave
// (lanes 60..63 idle): the half-plane of every kept neighbour, the number kept.  DETECT: a simulator has an exact distance tie
// that RVO2's visiting order decides if candidates of one agent shared a slot in the first sweep (strict ranks).
template <bool DETECT>
__device__ __forceinline__ void pair_sweep2(const Params& P, const Smem& s) {
    const int* kept = reinterpret_cast<const int*>(s.proj);
    const int tid = opaque_tid();
    const int wl = tid & (kWave - 1), g = wl / 10, slot = wl - g * 10;
    const int waves = (P.threads + kWave - 1) / kWave;
    const KdSmem k = DETECT ? kd_view(P, s) : KdSmem{};
    for (int q0 = (tid / kWave) * 6; q0 < P.nA; q0 += 6 * waves) {
        const int q = q0 + g;
        const bool lane_ok = wl < 60 && q < P.nA;
        const int e = lane_ok ? kept[q * 10 + slot] : -1;
        const bool valid = e >= 0;
        const unsigned long long vm = __ballot(valid);
        const int qq = lane_ok ? q : 0;
        const int ol = valid ? (e & 0xff) : qq;  // unused slots: a finite dummy (the agent against itself), not stored
        const bool robot_sim = (e >> 8) & 1;
        const float4 me = s.kin[qq];
        const float4 ot = s.kin[ol];
        const float rq_r = s.rview[qq], ro_r = s.rview[ol], rq_h = s.hview[qq], ro_h = s.hview[ol];
        const float rsum = (valid && robot_sim) ? rq_r + ro_r : rq_h + ro_h;
        if (lane_ok && slot == 0) s.count[q] = __popcll((vm >> (10 * g)) & 0x3ffull);
        if (valid)
            s.lines[q * kLineStride + slot] = make_half_plane(P.orca, me.x, me.y, me.z, me.w, ot.x, ot.y, ot.z, ot.w, rsum);
        if (DETECT) {  // more candidates claimed a slot than slots are filled: some share one, i.e. are equally far
            if (lane_ok && slot == 0 && reinterpret_cast<const int*>(k.dnext)[q] != (int)__popcll((vm >> (10 * g)) & 0x3ffull)) k.tie[q] = 1;
        }
    }
}

// Exact distance ties (rare: never in random scenes): work out RVO2's visiting order for the simulators that have one and rank
// their candidates again, ties by visiting order.  (Tried as a real call, __attribute__((noinline)): the mere presence of a call
// cost the 20-human rollout 4-5 % on every step — 62.3 vs 59.4 M env-steps/s instrumented — so it is inlined, and the few
// registers the rare path spills go to scratch.)  All threads of the workgroup (barriers inside).
template <bool COMPACT = false>
__device__ __forceinline__ void kd_resolve_ties(const Params& P, const Smem& s, const Lane& L, int kd_gen, int two_sweeps) {
    const KdSmem k = kd_scratch_view<COMPACT>(P, s);
    const float range_sq = P.orca.neighbor_dist * P.orca.neighbor_dist;
    if (L.lane < P.nA && k.tie[L.lane] != 0) kd_visit_order<COMPACT>(P, s, L, kd_gen);
    block_sync(P);
    int* kept = reinterpret_cast<int*>(s.proj);
    for (int p = L.lane; p < P.pairs; p += P.threads) {
        const int info = pair_info<COMPACT>(P, s, p);
        const int q = info & 0xff, c = (info >> 16) & 0xff, ol = (info >> 8) & 0xff;
        if (k.tie[q] == 0) continue;
        const int qb = q / P.A * P.A;
        const uint8_t* vq = k.visit + (size_t)q * k.row;
        const float mine = s.d2[p];
        const float* row = s.d2 + (p - c);
        const int my_visit = vq[ol - qb];
        int rank = 0;
        for (int kk = 0; kk < P.NC; ++kk) {
            const float v = row[kk];
            const int visit = vq[((pair_info<COMPACT>(P, s, p - c + kk) >> 8) & 0xff) - qb];
            rank += (v < range_sq ? 1 : 0) & ((v < mine ? 1 : 0) | ((v == mine ? 1 : 0) & (visit < my_visit ? 1 : 0)));
        }
        if (mine < range_sq && rank < P.orca.max_neighbors) {
            const bool robot_sim = (info >> 25) & 1;
            if (two_sweeps) {
                kept[q * 10 + rank] = ol | ((robot_sim ? 1 : 0) << 8);
            } else {
                const float4 me = s.kin[q];
                const float4 ot = s.kin[ol];
                const float rsum = robot_sim ? s.rview[q] + s.rview[ol] : s.hview[q] + s.hview[ol];
                s.lines[q * kLineStride + rank] = make_half_plane(P.orca, me.x, me.y, me.z, me.w, ot.x, ot.y, ot.z, ot.w, rsum);
            }
        }
    }
    block_sync(P);
    if (two_sweeps) {
        pair_sweep2<false>(P, s);
        block_sync(P);
    }
}

// ---------------------------------------------------------------------------------------------- ORCA phases
// Stage + pair phases + per-agent solve.  Called by all 64 lanes (contains barriers); on return every valid
// agent lane with solve == true holds its new velocity (ORCA.predict, orca.py:82-132).
// CN_PHASE_TIMING (compile time, profiling builds only): per-phase shader-clock accumulation inside the fused rollout
// (scripts/phase_probe.py).  Off in the product build: PhaseClock is empty and CN_TICK expands to nothing.
#ifdef CN_PHASE_TIMING
static __device__ unsigned long long cn_phase_cycles[16];  // (static: step_kernels.h is part of both translation units)
struct PhaseClock {
    unsigned long long last, acc[10];
};
#define CN_TICK(clk, k)                                                \
    do {                                                               \
        if (clk) {                                                     \
            const unsigned long long now_ = __builtin_readcyclecounter(); \
            (clk)->acc[k] += now_ - (clk)->last;                       \
            (clk)->last = now_;                                        \
        }                                                              \
    } while (0)
#else
struct PhaseClock {};
#define CN_TICK(clk, k) \
    do {                \
    } while (0)
#endif

// KD (compile time): the instantiation carries the kd-tree bookkeeping of simulators with more than 10 agents (kd_order.h);
// crowds of at most 9 humans run the one without it.
template <int MAXL, bool KD, bool COMPACT = false>
__device__ __forceinline__ void orca_phases(const Params& P, const Smem& s, const Lane& L, const AgentRegs& r,
                                            float robot_max_speed, bool solve, float& out_vx, float& out_vy,
                                            PhaseClock* clk = nullptr) {
    (void)clk;
    // preferred velocity: towards the goal, unit length once farther than 1 m (orca.py:113-115)
    // (COMPACT: the per-episode constants of the agent — goal, preferred speed, radius — are read from LDS where needed)
    const float max_speed = (L.a == 0) ? robot_max_speed : (float)(COMPACT ? (L.lane < P.nA ? s.vpref[L.lane] : 0.0) : r.vpref);
    auto preferred = [&](float& pref_x, float& pref_y) {
        const double2 goal = COMPACT ? s.goal2[L.lane] : make_double2(r.gx, r.gy);
        const double gdx = goal.x - r.px, gdy = goal.y - r.py;
        const double speed = norm2(gdx, gdy);
        pref_x = (float)(speed > 1.0 ? gdx / speed : gdx);
        pref_y = (float)(speed > 1.0 ? gdy / speed : gdy);
    };
    if (MAXL == 10 && P.NC == 20 && P.orca.max_neighbors == 10) {  // two-sweep pair phase: no neighbour in any slot yet
        int4* kept4 = reinterpret_cast<int4*>(s.proj);
        for (int i = L.lane; i * 4 < P.nA * 10; i += P.threads) kept4[i] = make_int4(-1, -1, -1, -1);
    }
    if (L.lane < P.nA) {
        s.kin[L.lane] = make_float4((float)r.px, (float)r.py, (float)r.vx, (float)r.vy);
        s.posd[L.lane] = make_double2(r.px, r.py);
        if (!COMPACT) {  // (COMPACT: written when the agent is loaded, stage_constants)
            s.rad[L.lane] = r.rad;
            s.hview[L.lane] = (float)(r.rad + 0.01 + step_param<COMPACT>(P, s, kParHSafety));
        }
        float pref_x, pref_y;
        preferred(pref_x, pref_y);
        s.sol[L.lane] = make_float4(pref_x, pref_y, max_speed, solve ? 1.0f : 0.0f);
        if (KD) {
            const KdSmem k = kd_view(P, s);
            k.tie[L.lane] = 0;
            reinterpret_cast<int*>(k.dnext)[L.lane] = 0;  // slots below 10 claimed by this agent's candidates (two-sweep pair phase)
        }
    }
    block_sync(P);
    // simulators of more than 10 agents: this step's kd-tree(s) and every simulator's permutation (kd_order.h); the visiting
    // order itself is only worked out further down if a simulator turns out to have an exact distance tie
    int kd_gen = 0;  // the generation of node lists that holds this step's tree
    if (KD) {
        const int g_last = *kd_view(P, s).gen;
        CN_TICK(clk, 0);
        if (P.E == 1 && P.threads == kWave) {
            kd_gen = kd_build_trees_wave(P, s, L, g_last);
            block_sync(P);  // (one wave: orders the builder's LDS records before the simulator lanes read them)
        } else {
            kd_gen = g_last ^ 1;
            kd_build_trees(P, s, L, kd_gen);
        }
        CN_TICK(clk, 4);  // (probe builds: the tree build is booked under "robot action publish")
        kd_update_orders(P, s, L, kd_gen);
        if (L.lane == 0) *kd_view(P, s).gen = kd_gen;
    }
    CN_TICK(clk, 0);

    // pairs-1: squared distances, self.pos - other.pos (Appendix A.2)
    for (int p = L.lane; p < P.pairs; p += P.threads) {
        const int info = pair_info<COMPACT>(P, s, p);
        const float4 me = s.kin[info & 0xff];
        const float4 ot = s.kin[(info >> 8) & 0xff];
        const float dx = me.x - ot.x, dy = me.y - ot.y;
        s.d2[p] = ((info >> 24) & 1) ? dx * dx + dy * dy : std::numeric_limits<float>::infinity();
    }
    block_sync(P);
    CN_TICK(clk, 1);

    // pairs-2: neighbour slot = stable rank by (distSq, visit order) among the in-range candidates, which
    // is what RVO2's sorted insertion with strict '<' produces; slots >= maxNeighbors fall off the list.
    const float range_sq = P.orca.neighbor_dist * P.orca.neighbor_dist;
    // BASELINE configs[3]'s crowd (20 candidates per agent, 10 kept): the candidate row comes in as five 16-byte reads
    // issued together (the scalar loop waited for LDS once per two candidates: ten round trips per pass of 64 pairs), and
    // the half-plane is computed in a second sweep over the (agent, kept slot) lanes only — 210 of the 420 ordered pairs,
    // four passes of a wave instead of seven.  Same comparisons and the same half-plane arithmetic: bit-identical.
    const bool two_sweeps = MAXL == 10 && P.NC == 20 && P.orca.max_neighbors == 10;
    if (two_sweeps) {
        // kept [nA][10]: candidate lane | robot's-sim bit << 8 of the pair that ranks there, -1 = no such neighbour (cleared in
        // the stage phase; proj is free until the solve).  A pair inside the range ranks by (v < mine) | (v == mine & k < c)
        // alone: every candidate that precedes it is inside the range too — 4 vector instructions per candidate instead of 7;
        // the ranks of an agent's in-range candidates are a permutation of 0 .. within - 1, so the neighbours kept are
        // exactly the filled slots and their number falls out of the second sweep's ballot.
        // With the kd bookkeeping (always, at 20 candidates) the rank counts STRICTLY nearer candidates only — 2 vector
        // instructions per candidate instead of 4-5: candidates at exactly the same distance then share a rank and a slot, which
        // the second sweep notices (more candidates claimed a slot below 10 than slots are filled) and kd_resolve_ties ranks
        // that agent's candidates again, ties by RVO2's visiting order.
        int* kept = reinterpret_cast<int*>(s.proj);
        int* const claimed = KD ? reinterpret_cast<int*>(kd_view(P, s).dnext) : nullptr;
        for (int p = L.lane; p < P.pairs; p += P.threads) {
            const int info = pair_info<COMPACT>(P, s, p);
            const int c = (info >> 16) & 0xff;
            const float mine = s.d2[p];
            const float4* row4 = reinterpret_cast<const float4*>(s.d2 + (p - c));
            float v[20];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float4 t = row4[j];
                v[4 * j] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
            }
            int rank = 0;
            if (KD) {
                // squared distances are +0 .. +inf: their bit patterns order like the floats, and bit 31 of the 32-bit difference
                // says v < mine.  v_sub_u32 + v_alignbit_b32 (shift the sign into a 20-bit word) per candidate and one popcount,
                // instead of v_cmp -> vcc -> v_cndmask / v_addc with a two-state hazard s_nop between each pair (gfx950): 41
                // issue slots per pass instead of 60, nothing through VCC.
                const uint32_t mb = __float_as_uint(mine);
                uint32_t nearer = 0u;
#pragma unroll
                for (int k = 0; k < 20; ++k) nearer = __builtin_amdgcn_alignbit(nearer, __float_as_uint(v[k]) - mb, 31);
                rank = __popc(nearer);
            } else {
#pragma unroll
                for (int k = 0; k < 20; ++k) rank += ((v[k] < mine) | ((v[k] == mine) & (k < c))) ? 1 : 0;
            }
            if (mine < range_sq && rank < 10) {
                kept[(info & 0xff) * 10 + rank] = ((info >> 8) & 0xff) | (((info >> 25) & 1) << 8);
                if (KD) atomicAdd(claimed + (info & 0xff), 1);  // (LDS, no return value)
            }
        }
        block_sync(P);
        if (KD)
            pair_sweep2<true>(P, s);
        else
            pair_sweep2<false>(P, s);
    } else
    for (int p = L.lane; p < P.pairs; p += P.threads) {
        const int info = pair_info<COMPACT>(P, s, p);
        const int q = info & 0xff, c = (info >> 16) & 0xff;
        const float mine = s.d2[p];
        const float* row = s.d2 + (p - c);
        int rank = 0, within = 0, same = 0;
        for (int k = 0; k < P.NC; ++k) {  // (bitwise, not short-circuit: no branch per candidate)
            const float v = row[k];
            const int in = v < range_sq ? 1 : 0;
            within += in;
            same += v == mine ? 1 : 0;  // itself included
            rank += in & ((v < mine ? 1 : 0) | ((v == mine ? 1 : 0) & (k < c ? 1 : 0)));
        }
        if (KD && mine < range_sq && same > 1) kd_view(P, s).tie[q] = 1;  // an exact tie: RVO2's kd-tree visiting order decides
        if (c == 0) s.count[q] = within < P.orca.max_neighbors ? within : P.orca.max_neighbors;
        if (mine < range_sq && rank < P.orca.max_neighbors) {
            const int ol = (info >> 8) & 0xff;
            const float4 me = s.kin[q];
            const float4 ot = s.kin[ol];
            const bool robot_sim = (info >> 25) & 1;
            const float rsum = robot_sim ? s.rview[q] + s.rview[ol] : s.hview[q] + s.hview[ol];
            s.lines[q * kLineStride + rank] =
                make_half_plane(P.orca, me.x, me.y, me.z, me.w, ot.x, ot.y, ot.z, ot.w, rsum);
        }
    }
    block_sync(P);
    if (KD) {
        const KdSmem k = kd_view(P, s);
        const bool my_tie = L.lane < P.nA && k.tie[L.lane] != 0;
        if (block_sync_or(P, my_tie ? 1 : 0)) kd_resolve_ties<COMPACT>(P, s, L, kd_gen, two_sweeps ? 1 : 0);
    }
    CN_TICK(clk, 2);

    out_vx = 0.0f, out_vy = 0.0f;
    float rx = 0.0f, ry = 0.0f;
    int n = 0, fail = 0;
    if (MAXL == 5) {
        // candidates: lane = (agent, half-plane)
        for (int p = L.lane; p < P.nA * MAXL; p += P.threads) {
            const int q = p / MAXL, k = p - q * MAXL;
            const float4 so = s.sol[q];
            const float4* lq = s.lines + q * kLineStride;
            s.cand2[q * kLineStride + k] = lp_line_candidate<MAXL - 1>(lq[k], lq, k, so.z, so.x, so.y, false);
            if (k == 0) {
                float sx, sy;
                lp_start_point(so.z, so.x, so.y, sx, sy);
                s.res[q] = make_float4(sx, sy, 0.0f, 0.0f);
            }
        }
        block_sync(P);
        if (solve) {
            n = s.count[L.lane];
            const float4 start = s.res[L.lane];
            rx = start.x, ry = start.y;
            fail = lp_planar_scan<MAXL>(s.lines + L.lane * kLineStride, s.cand2 + L.lane * kLineStride, n, rx, ry);
        }
    } else {
        lp_planar_tri(s.lines, s.count, s.sol, s.res, P.nA, P.threads);  // every thread: lane = (agent, third of its half-planes)
        block_sync(P);
        if (solve) {
            n = s.count[L.lane];
            const float4 got = s.res[L.lane];
            rx = got.x, ry = got.y;
            fail = __float_as_int(got.z);
        }
    }
    CN_TICK(clk, 3);
    const bool need = solve && fail < n;
#ifdef CN_PHASE_TIMING
    if (clk) clk->acc[9] += __popcll(__ballot(need));  // agents in the fallback
#endif
    if (block_sync_or(P, need ? 1 : 0)) {  // some agent of this workgroup was infeasible: compact them
        if (L.lane < kWave) {  // (agent lanes live in wave 0)
            const unsigned long long nm = __ballot(need);
            if (need) {
                if (MAXL == 10) s.res[L.lane] = make_float4(rx, ry, __int_as_float(fail), 0.0f);
                s.todo[__popcll(nm & ((1ull << L.lane) - 1ull))] = L.lane;
            }
            if (L.lane == 0) s.todo[P.nA] = __popcll(nm);
        }
        block_sync(P);
        if (MAXL == 5) {
            constexpr int kPairs = 10;  // MAXL (MAXL - 1) / 2 projections and as many candidates per infeasible agent
            const int items = s.todo[P.nA] * kPairs;
            for (int p = L.lane; p < items; p += P.threads) {  // projections: lane = (agent, i, j)
                const int t = p / kPairs, m = p - t * kPairs;
                const int a = s.todo[t];
                const int i = lp3_program_of(m), j = m - i * (i - 1) / 2;
                const float4* la = s.lines + a * kLineStride;
                s.proj[a * kLineStride + m] = lp3_project(la[i], la[j]);
            }
            block_sync(P);
            for (int p = L.lane; p < items; p += P.threads) {  // their candidates: lane = (agent, i, k)
                const int t = p / kPairs, m = p - t * kPairs;
                const int a = s.todo[t];
                const int i = lp3_program_of(m), base = i * (i - 1) / 2;
                const float4 li = s.lines[a * kLineStride + i];
                const float4* pa = s.proj + a * kLineStride + base;
                s.cand3[a * kLineStride + m] = lp_line_candidate<3>(pa[m - base], pa, m - base, s.sol[a].z, -li.w, li.z, true);
            }
            block_sync(P);
            if (need)
                lp3_scan(s.lines + L.lane * kLineStride, s.proj + L.lane * kLineStride, s.cand3 + L.lane * kLineStride, n, fail,
                         max_speed, rx, ry);
        } else {
            // (the lazy fallback's candidate rows — 7 agents x 9 float4 per wave — live in d2, free after the pair phases: enough
            // for one wave of a crowd of 12+ agents; otherwise the shuffle-round form)
            if (P.threads == kWave && P.pairs * 4 >= kLazyCandFloat4 * 16)
                lp_relaxed_lazy<10, COMPACT>(s.lines, s.proj, reinterpret_cast<float4*>(s.d2), s.count, s.sol, s.res, s.todo,
                                             s.todo[P.nA], P.threads);
            else
                lp_relaxed_coop<10>(s.lines, s.count, s.sol, s.res, s.todo, s.todo[P.nA]);
            block_sync(P);
            if (need) {
                const float4 got = s.res[L.lane];
                rx = got.x, ry = got.y;
            }
        }
    }
    out_vx = rx, out_vy = ry;
    CN_TICK(clk, 8);
}

struct StepResult {  // meaningful on the robot lane
    double reward, dmin, ax, ay;
    uint8_t done, info;
};

// One transition for the lane's agent (crowd_sim.py:317-420).  `r` is updated in place when update != 0.
// new_vx/new_vy: the velocity this lane's agent chose (float32 for ORCA agents, the action for the robot).
// Must be called by all 64 lanes (contains workgroup barriers).
// UNI (compile time): the robot may be a unicycle.  The holonomic instantiation carries none of that code — it sits
// inside the fused rollout loop, where 20 extra VGPRs and a few dead branches cost 7 % (712 -> 665 M env-steps/s).
template <int MAXL, bool UNI, bool KD, bool COMPACT = false>
__device__ __forceinline__ void step_core(const Params& P, const Smem& s, const Lane& L, AgentRegs& r,
                                          double& gtime, float robot_max_speed, const double* ext_action,
                                          int update, StepResult& res, double& new_vx, double& new_vy,
                                          double* theta_io = nullptr, PhaseClock* clk = nullptr, const float* known_vel = nullptr,
                                          const double* robot_action_regs = nullptr /* the robot lane's action, in registers */,
                                          const float* lane_vel_regs = nullptr /* this lane's entry of known_vel, requested earlier */) {
    (void)clk;
    float ovx = 0.0f, ovy = 0.0f;
    if (known_vel != nullptr) {
        // the humans' ORCA velocities of THIS state are known already ([B][A][2], orca_kernel's output: sarl_decide_step_kernel
        // computed them behind the previous transition for the decision's lookahead — the same function of the same state);
        // what the phases below read from LDS besides them: the agents' float64 positions and radii
        if (L.lane < P.nA) {
            s.posd[L.lane] = make_double2(r.px, r.py);
            if (!COMPACT) s.rad[L.lane] = r.rad;
        }
        if (L.valid && L.a > 0) {
            ovx = lane_vel_regs ? lane_vel_regs[0] : known_vel[2 * L.gi];
            ovy = lane_vel_regs ? lane_vel_regs[1] : known_vel[2 * L.gi + 1];
        }
    } else {
        orca_phases<MAXL, KD, COMPACT>(P, s, L, r, robot_max_speed, L.valid && (L.a > 0 || P.robot_orca), ovx, ovy, clk);
    }
    new_vx = ovx;
    new_vy = ovy;
    // unicycle robot (ActionRot v, r): the collision test uses v (cos, sin)(r + theta) (crowd_sim.py:339-341), the
    // move is compute_position's (agent.py:115-118)
    const bool unicycle = UNI && P.robot_unicycle && !P.robot_orca && L.valid && L.a == 0;
    double rot_v = 0.0, rot_r = 0.0, theta0 = 0.0;
    if (L.valid && L.a == 0) {
        if (!P.robot_orca) {
            new_vx = robot_action_regs ? robot_action_regs[0] : ext_action[2 * (size_t)L.env];
            new_vy = robot_action_regs ? robot_action_regs[1] : ext_action[2 * (size_t)L.env + 1];
        }
        if (unicycle) {
            rot_v = new_vx, rot_r = new_vy, theta0 = *theta_io;
            new_vx = rot_v * cos(rot_r + theta0);
            new_vy = rot_v * sin(rot_r + theta0);
        }
        s.act[L.lane] = make_double2(new_vx, new_vy);
    }
    block_sync(P);
    CN_TICK(clk, 4);

    // One float64 distance per agent lane, computed branch-free so that humans and the robot share the
    // instruction stream:
    //   human: swept robot-human distance over the step, human's CURRENT velocity vs the robot's NEW action
    //          = point_to_segment_dist(px, py, ex, ey, 0, 0) - r_h - r_r      (crowd_sim.py:331-351)
    //   robot: distance of its end position to its goal                       (crowd_sim.py:364-366)
    double goal_dist = 0.0;
    if (L.valid) {
        const bool human = L.a > 0;
        const double2 rp = s.posd[L.ebase];
        const double2 act = s.act[L.ebase];
        const double x1 = r.px - rp.x, y1 = r.py - rp.y;
        const double wx = r.vx - act.x, wy = r.vy - act.y;
        const double c_dt = step_param<COMPACT>(P, s, kParDt);
        const double2 cp = closest_point(x1, y1, wx, wy, c_dt);
        double endx = r.px + new_vx * c_dt, endy = r.py + new_vy * c_dt;
        if (unicycle) {
            const double th = theta0 + rot_r;
            endx = r.px + cos(th) * rot_v * c_dt;
            endy = r.py + sin(th) * rot_v * c_dt;
        }
        const double2 goal = COMPACT ? s.goal2[L.lane] : make_double2(r.gx, r.gy);
        const double d = norm2(human ? cp.x : endx - goal.x, human ? cp.y : endy - goal.y);
        if (human) {
            s.closest[L.lane] = d - (COMPACT ? s.rad[L.lane] : r.rad) - s.rad[L.ebase];
        } else {
            goal_dist = d;
        }
    }
    block_sync(P);
    CN_TICK(clk, 5);

    res.done = 0;
    if (L.valid && L.a == 0) {
        // the reference stops scanning at the first colliding human (dmin keeps the minimum seen before it)
        double dmin = std::numeric_limits<double>::infinity();
        bool collision = false;
        for (int i = 1; i < P.A; ++i) {
            const double c = s.closest[L.lane + i];
            const bool hit = c < 0.0;
            dmin = (!collision && !hit && c < dmin) ? c : dmin;
            collision = collision || hit;
        }
        const bool reaching = goal_dist < (COMPACT ? s.rad[L.lane] : r.rad);
        const double c_ddist = step_param<COMPACT>(P, s, kParDDist);
        if (gtime >= step_param<COMPACT>(P, s, kParLimit) - 1.0) {
            res.reward = 0.0, res.done = 1, res.info = CN_TIMEOUT;
        } else if (collision) {
            res.reward = step_param<COMPACT>(P, s, kParCollision), res.done = 1, res.info = CN_COLLISION;
        } else if (reaching) {
            res.reward = step_param<COMPACT>(P, s, kParSuccess), res.done = 1, res.info = CN_REACH_GOAL;
        } else if (dmin < c_ddist) {
            res.reward = (dmin - c_ddist) * step_param<COMPACT>(P, s, kParDFactor) * step_param<COMPACT>(P, s, kParDt);
            res.done = 0, res.info = CN_DANGER;
        } else {
            res.reward = 0.0, res.done = 0, res.info = CN_NOTHING;
        }
        res.dmin = dmin;
        res.ax = unicycle ? rot_v : new_vx, res.ay = unicycle ? rot_r : new_vy;
        if (update) gtime += step_param<COMPACT>(P, s, kParDt);
    }
    if (update && L.valid) {  // Agent.step (agent.py:127-135)
        const double c_dt = step_param<COMPACT>(P, s, kParDt);
        if (unicycle) {
            const double th = theta0 + rot_r;
            r.px = r.px + cos(th) * rot_v * c_dt;
            r.py = r.py + sin(th) * rot_v * c_dt;
            const double theta1 = python_fmod(theta0 + rot_r, 2 * 3.141592653589793);
            r.vx = rot_v * cos(theta1);
            r.vy = rot_v * sin(theta1);
            *theta_io = theta1;
        } else {
            r.px = r.px + new_vx * c_dt;
            r.py = r.py + new_vy * c_dt;
            r.vx = new_vx;
            r.vy = new_vy;
        }
    }
    CN_TICK(clk, 6);
}

// ---------------------------------------------------------------------------------------------- kernels

template <int MAXL, bool KD>
__global__ __launch_bounds__(kMaxBlock) void orca_kernel(Params P, StateView S, float* out_vel) {
    const Smem s = carve<MAXL>(P);
    const Lane L = lane_of(P);
    AgentRegs r = {};
    if (L.valid) load_agent(S, L.gi, r);
    float robot_max_speed;
    load_robot_view(P, S, s, L, r, robot_max_speed);
    build_pairs(P, s);
    if (KD) kd_load(P, S, s, L);
    float vx, vy;
    orca_phases<MAXL, KD>(P, s, L, r, robot_max_speed, L.valid, vx, vy);
    if (KD) kd_store(P, S, s, L);
    if (L.valid) {
        out_vel[2 * L.gi] = vx;
        out_vel[2 * L.gi + 1] = vy;
        if (L.a == 0) S.rsim_valid[L.env] = 1;
    }
}

template <int MAXL, bool UNI, bool KD>
__global__ __launch_bounds__(kMaxBlock) void step_kernel(Params P, StateView S, StepIo io) {
    const Smem s = carve<MAXL>(P);
    const Lane L = lane_of(P);
    AgentRegs r = {};
    if (L.valid) load_agent(S, L.gi, r);
    float robot_max_speed = 0.0f;
    if (P.robot_orca) load_robot_view(P, S, s, L, r, robot_max_speed);
    build_pairs(P, s);
    if (KD) kd_load(P, S, s, L);
    double gtime = (L.valid && L.a == 0) ? S.gtime[L.env] : 0.0;
    const AgentRegs before = r;

    double theta = (L.valid && L.a == 0) ? S.theta[L.env] : 0.0;
    StepResult res;
    double nvx, nvy;
    step_core<MAXL, UNI, KD>(P, s, L, r, gtime, robot_max_speed, io.action, io.update, res, nvx, nvy, &theta);
    if (KD) kd_store(P, S, s, L);  // (a lookahead rebuilds the humans' trees too: the reference's onestep_lookahead runs doStep)
    if (!L.valid) return;

    if (L.a == 0) {
        io.reward[L.env] = res.reward;
        io.done[L.env] = res.done;
        io.info[L.env] = res.info;
        if (io.dmin) io.dmin[L.env] = res.dmin;
        if (io.action_out) {
            io.action_out[2 * (size_t)L.env] = res.ax;
            io.action_out[2 * (size_t)L.env + 1] = res.ay;
        }
        if (io.update) {
            S.gtime[L.env] = gtime;
            S.theta[L.env] = theta;
        }
        if (P.robot_orca) S.rsim_valid[L.env] = 1;
    }
    if (io.orca_vel) {
        io.orca_vel[2 * L.gi] = (float)nvx;
        io.orca_vel[2 * L.gi + 1] = (float)nvy;
    }
    if (io.update) {
        S.pos[L.gi] = make_double2(r.px, r.py);
        S.vel[L.gi] = make_double2(r.vx, r.vy);
    }
    if (io.obs && L.a > 0) {
        // update: get_observable_state after the move; else get_next_observable_state (agent.py:63-74)
        double* o = io.obs + ((size_t)L.env * (P.A - 1) + (L.a - 1)) * 5;
        if (io.update) {
            o[0] = r.px, o[1] = r.py, o[2] = r.vx, o[3] = r.vy;
        } else {
            o[0] = before.px + nvx * P.dt, o[1] = before.py + nvy * P.dt, o[2] = nvx, o[3] = nvy;
        }
        o[4] = r.rad;
    }
}

}  // namespace cn
