// The rollout kernels of the env translation unit (crowdnav_amd.hip): the episode bookkeeping of explorer.py:50-72 (records,
// EpisodeBook, the CN_*_EPISODE rules), the launch epilogue, and the four kernels whose body is rollout_body.inc.  The transition
// itself is step_kernels.h's step_core; where the next scenario comes from is scenario_ring.h.
#pragma once
#include "scenario_ring.h"

namespace cn {

// explorer.py:50-72: the finished episode's record (robot lane)
__device__ __forceinline__ void write_record(const cn_rollout_io& io, int env, int ep_count, int info, int cur_steps,
                                             double cur_return, double time, int cur_danger, double cur_dsum) {
    if (io.record_capacity > 0) {
        const size_t k = (size_t)env * io.record_capacity + (ep_count % io.record_capacity);
        if (io.ep_outcome) io.ep_outcome[k] = (uint8_t)info;
        if (io.ep_steps) io.ep_steps[k] = cur_steps;
        if (io.ep_return) io.ep_return[k] = cur_return;
        if (io.ep_time) io.ep_time[k] = time;
        if (io.ep_danger) io.ep_danger[k] = cur_danger;
        if (io.ep_danger_dmin_sum) io.ep_danger_dmin_sum[k] = cur_dsum;
    }
}

// ---- the episode bookkeeping of explorer.py:50-72, each piece stated once ------------------------------------------
// What an env carries from step to step and from call to call.  The generic kernels keep it in the robot lane's registers,
// the shard's kernel in LDS between steps (EpisodeLds), the fused kernels on every lane of the env.
struct EpisodeBook {
    double gtime, cur_return, cur_dsum;  // global_time; the running episode's discounted return and sum of Danger min_dist
    int cur_steps, cur_danger;           // ... its transitions and its Danger steps
    int ep_count, ring_filled, state;    // episodes finished; the launch-time ring fill level; kRunning / kWaitingScenario / kRetired
};
struct EpisodeLds {  // at Smem::disc + 8 (COMPACT: one robot per workgroup)
    EpisodeBook book;
    unsigned int transitions;
    unsigned int dyn_total;  // dynamic schedule: transitions of all the visits this workgroup ran (not a register held across them)
};
static_assert(sizeof(EpisodeLds) <= 8 * (kCompactScratchDoubles - 8), "EpisodeLds outgrew its LDS slot");

// The four pieces below are MACROS, expanded in rollout_body.inc and rollout_fused.h, for the reason rollout_body.inc is
// included text: as __device__ __forceinline__ functions (the book by reference, or returned by value) hipcc gave every
// rollout_kernel instantiation another instruction stream with one to seventeen more spilled SGPRs, and the generic
// 10-half-plane kernel lost 1.3 % (profiles/episode_book_refactor.txt); expanded as text they compile to the code the kernels
// had when each spelled them out.  `io` is a cn_rollout_io (a local copy of the device block), `S` a StateView expression.
//
// The book of env `env` as the previous call left it.  Straight-line loads, none under another's result: a caller that wants
// them issued in one batch with its other loads expands this unconditionally on a clamped index (rollout_fused.h).
#define CN_LOAD_EPISODE(P, e, S, io, ring_filled_in, env)                                         \
    do {                                                                                          \
        (e).gtime = (S).gtime[env];                                                               \
        (e).state = (io).active[env];                                                             \
        (e).ep_count = (io).ep_count[env];                                                        \
        (e).ring_filled = (ring_filled_in)[env];                                                  \
        (e).cur_steps = (io).cur_steps[env];                                                      \
        (e).cur_return = (io).cur_return[env];                                                    \
        (e).cur_danger = (io).cur_danger ? (io).cur_danger[env] : 0;                              \
        (e).cur_dsum = (io).cur_danger_dmin_sum ? (io).cur_danger_dmin_sum[env] : 0.0;            \
        /* a launch looks at most ring_depth scenarios ahead, however far the (lagged) fill has got */ \
        (e).ring_filled = min((e).ring_filled, ring_next_ordinal((e).ep_count, (e).state) + (P).ring_depth); \
    } while (0)
// ... and as this call leaves it (robot lane), with the robot's heading, the "robot's simulator exists" mark and ep_word;
// beside it the agent's own state (every agent lane)
#define CN_STORE_EPISODE(P, S, io, env, e, theta)                                                 \
    do {                                                                                          \
        (S).gtime[env] = (e).gtime;                                                               \
        (S).theta[env] = (theta);                                                                 \
        if ((P).robot_orca) (S).rsim_valid[env] = 1;                                              \
        (io).active[env] = (uint8_t)(e).state;                                                    \
        (io).ep_count[env] = (e).ep_count;                                                        \
        (io).cur_steps[env] = (e).cur_steps;                                                      \
        (io).cur_return[env] = (e).cur_return;                                                    \
        if ((io).cur_danger) (io).cur_danger[env] = (e).cur_danger;                               \
        if ((io).cur_danger_dmin_sum) (io).cur_danger_dmin_sum[env] = (e).cur_dsum;               \
        (S).ep_word[env] = ((e).ep_count << 2) | (e).state;                                       \
    } while (0)
#define CN_STORE_AGENT(S, gi, r)                                                                  \
    do {                                                                                          \
        (S).pos[gi] = make_double2((r).px, (r).py);                                               \
        (S).vel[gi] = make_double2((r).vx, (r).vy);                                               \
        (S).goal[gi] = make_double2((r).gx, (r).gy);                                              \
        (S).rv[gi] = make_double2((r).rad, (r).vpref);                                            \
    } while (0)

// One transition of the running episode: `disc` is gamma ** (cur_steps * dt * v_pref) of THIS step.
#define CN_BOOK_TRANSITION(e, disc, reward, info, dmin)                                           \
    do {                                                                                          \
        (e).cur_return = (e).cur_return + (disc) * (reward); /* python sum(): left to right */    \
        ++(e).cur_steps;                                                                          \
        if ((info) == CN_DANGER) {                                                                \
            ++(e).cur_danger;                                                                     \
            (e).cur_dsum += (dmin);                                                               \
        }                                                                                         \
    } while (0)

// Episode end: append the record (the lane with `write`), start the book afresh, pick the next episode.  The decision is the
// env's new state, (e).state: kRetired; kWaitingScenario (ring ran dry, or this scenario is still being generated: pause until a
// later launch); kRunning = go on with the scenario of ordinal (e).ep_count — then, and only then, the statement
// NEXT_SCENARIO runs: what the kernel does to take it from ring slot (e).ep_count % P.ring_mod.
#define CN_END_EPISODE(P, S, io, env, write, time_limit, info, e, NEXT_SCENARIO)                                              \
    do {                                                                                                                      \
        if (write)                                                                                                            \
            write_record(io, env, (e).ep_count, info, (e).cur_steps, (e).cur_return, ((info) == CN_TIMEOUT) ? (time_limit) : (e).gtime, \
                         (e).cur_danger, (e).cur_dsum);                                                                       \
        (e).cur_steps = 0, (e).cur_return = 0.0, (e).cur_danger = 0, (e).cur_dsum = 0.0;                                      \
        (e).gtime = 0.0;                                                                                                      \
        ++(e).ep_count;                                                                                                       \
        if (past_episode_limit(io, episode_id(io, env, (e).ep_count))) {                                                      \
            (e).state = kRetired;                                                                                             \
        } else if (scenario_ready(P, S, env, (e).ep_count, (e).ring_filled)) {                                                \
            NEXT_SCENARIO;                                                                                                    \
        } else {                                                                                                              \
            (e).state = kWaitingScenario;                                                                                     \
        }                                                                                                                     \
    } while (0)

// ---------------------------------------------------------------------------------------------- launch epilogue
// Behind every rollout launch there used to be three more kernels on the stream: rollout_finish_kernel (the transitions
// counter), records_pack_kernel (the shard's record blocks) and records_summary_kernel (explorer.py:74-90) — 18 us of
// kernels plus their boundaries behind a 106 us launch in the driver's 20-step shape.  They are the tail of the rollout
// kernel now: every workgroup leaves its share (its envs' record blocks; the sums over its envs' record rings and its
// transitions as one partial record), takes an arrival ticket of its group (workgroup b -> counter b % 32: 64 arrivals per counter at
// 2048 workgroups; every counter on its own 256-byte line — nine counters in ONE line serialised all 2048 arrivals of a
// 1-step launch: 35 us instead of 17), the last arrival of a group adds the group's partial sums in workgroup order and
// arrives at the top counter, and the last of those writes the results.  The summation
// order is a function of the workgroup indices only, never of the arrival order: the same bits on every run.
// Hand-off between workgroups (MI355X_MICROARCH.md, inter-workgroup visibility): payload as 8-byte agent-scope atomic
// stores (write-through), s_waitcnt vmcnt(0), then the ticket (agent-scope RMW); the reader loads the payload with
// agent-scope atomic loads after its own ticket came back.  No L2 write-back / L1 invalidate fences.
__device__ __forceinline__ void agent_store(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double agent_load(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}

// scratch: LDS, at least (E * (CN_SUMMARY_FIELDS + 1) + 1) doubles, free after the last barrier of the step loop.
// Called by every thread of the workgroup (contains barriers); `transitions` / `ep_count` are read on the robot lanes.
//   extra_env (>= 0, robot lanes): an env that is NOT part of this launch (the 3-of-4 schedule's last sub-launch) whose record
//   ring this workgroup adds to its sums, so that the statistics the launch leaves behind cover every env of the engine
__device__ __forceinline__ void rollout_epilogue(const Params& P, const StateView& S, const cn_rollout_io& io, const Lane& L,
                                                 bool robot, unsigned int transitions, int ep_count, double* scratch,
                                                 int extra_env = -1) {
    constexpr int F = CN_SUMMARY_FIELDS + 1;  // the eight sums + this launch's transitions (exact in a double)
    const int tid = threadIdx.x;
    const int cap = io.record_capacity;
    const int held = ep_count < cap ? ep_count : cap;
    if (robot && io.blocks) {  // cn_rollout_records' block of this env
        const int K = io.blocks_records;
        double* blk = io.blocks + (size_t)L.env * (1 + (size_t)K * CN_RECORD_FIELDS);
        blk[0] = (double)ep_count;
        for (int j = 0; j < K; ++j) {
            double* rec = blk + 1 + (size_t)j * CN_RECORD_FIELDS;
            const bool have = j < held;
            const size_t k = (size_t)L.env * cap + j;
            rec[0] = (have && io.ep_outcome) ? (double)io.ep_outcome[k] : 0.0;
            rec[1] = (have && io.ep_steps) ? (double)io.ep_steps[k] : 0.0;
            rec[2] = (have && io.ep_return) ? io.ep_return[k] : 0.0;
            rec[3] = (have && io.ep_time) ? io.ep_time[k] : 0.0;
            rec[4] = (have && io.ep_danger) ? (double)io.ep_danger[k] : 0.0;
            rec[5] = (have && io.ep_danger_dmin_sum) ? io.ep_danger_dmin_sum[k] : 0.0;
        }
    }
    if (robot && io.env_transitions) io.env_transitions[L.env] += (uint64_t)transitions;  // (ABI v6) this env's own counter
    const bool want = io.summary != nullptr;  // uniform over the launch
    // nothing job-wide asked for: the launch ends here — no partial sums, no arrival tickets, no hand-off between workgroups
    // (eight dependent memory round trips of the LAST wave, ~9 of the 113 us of a 20-step launch)
    if (!want && io.transitions == nullptr) return;
    if (robot) {  // this env's sums over its record ring (cn_records_summary's fields) + its transitions
        double acc[F] = {};
        acc[F - 1] = (double)transitions;
        if (want) {
            acc[0] = (double)ep_count;
            acc[1] = (double)held;
            for (int j = 0; j < held; ++j) {
                const size_t k = (size_t)L.env * cap + j;
                const int outcome = io.ep_outcome ? (int)io.ep_outcome[k] : 0;
                acc[2] += outcome == CN_REACH_GOAL ? 1.0 : 0.0;
                acc[3] += outcome == CN_COLLISION ? 1.0 : 0.0;
                acc[4] += outcome == CN_TIMEOUT ? 1.0 : 0.0;
                acc[5] += (outcome == CN_REACH_GOAL && io.ep_time) ? io.ep_time[k] : 0.0;
                acc[6] += io.ep_return ? io.ep_return[k] : 0.0;
                acc[7] += io.ep_danger ? (double)io.ep_danger[k] : 0.0;
            }
            if (extra_env >= 0) {
                const int n2 = io.ep_count[extra_env], held2 = n2 < cap ? n2 : cap;
                acc[0] += (double)n2;
                acc[1] += (double)held2;
                for (int j = 0; j < held2; ++j) {
                    const size_t k = (size_t)extra_env * cap + j;
                    const int outcome = io.ep_outcome ? (int)io.ep_outcome[k] : 0;
                    acc[2] += outcome == CN_REACH_GOAL ? 1.0 : 0.0;
                    acc[3] += outcome == CN_COLLISION ? 1.0 : 0.0;
                    acc[4] += outcome == CN_TIMEOUT ? 1.0 : 0.0;
                    acc[5] += (outcome == CN_REACH_GOAL && io.ep_time) ? io.ep_time[k] : 0.0;
                    acc[6] += io.ep_return ? io.ep_return[k] : 0.0;
                    acc[7] += io.ep_danger ? (double)io.ep_danger[k] : 0.0;
                }
            }
        }
        const int el = L.ebase / P.A;
#pragma unroll
        for (int f = 0; f < F; ++f) scratch[el * F + f] = acc[f];
    }
    block_sync(P);
    const int f0 = want ? 0 : F - 1;  // without a summary only the transitions travel
    if (tid >= f0 && tid < F) {  // the workgroup's envs in env order
        double t = 0.0;
        for (int el = 0; el < P.E; ++el)
            if ((int)blockIdx.x * P.E + el < P.B) t += scratch[el * F + tid];
        agent_store(S.wg_partial + (size_t)blockIdx.x * F + tid, t);
    }
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "rollout_epilogue orders its payload stores before the ticket with s_waitcnt vmcnt(0): on gfx9 (gfx950) vmcnt counts stores; gfx10+ counts them in vscnt - use release / acquire atomics there"
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this lane's payload has left before the ticket is taken
    block_sync(P);
    int* const flag = reinterpret_cast<int*>(scratch + P.E * F);
    const int n_wg = (int)gridDim.x;
    const int g = blockIdx.x % kEpilogueGroups;
    const int members = (n_wg - g + kEpilogueGroups - 1) / kEpilogueGroups;  // workgroups b with b % groups == g
    if (tid == 0)
        flag[0] = __hip_atomic_fetch_add(&S.tickets[g * kTicketStride], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                  (unsigned)(members - 1);
    block_sync(P);
    if (!flag[0]) return;
    // last arrival of group g: the group's sums, members in index order (lane l: members l, l + 64, ..; lanes by a fixed tree)
    if (tid < kWave) {
        double acc[F] = {};
        for (int m = tid; m < members; m += kWave) {
            const double* p = S.wg_partial + (size_t)(g + kEpilogueGroups * m) * F;
#pragma unroll
            for (int f = 0; f < F; ++f)
                if (f >= f0) acc[f] += agent_load(p + f);
        }
#pragma unroll
        for (int f = 0; f < F; ++f) {
            if (f < f0) continue;
            double v = acc[f];
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
            if (tid == 0) agent_store(S.group_partial + g * F + f, v);
        }
    }
    const int groups = n_wg < kEpilogueGroups ? n_wg : kEpilogueGroups;
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        flag[1] = __hip_atomic_fetch_add(&S.tickets[kEpilogueGroups * kTicketStride], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(groups - 1);
    }
    block_sync(P);
    if (!flag[1]) return;
    // last arrival of all: results out, counters back to zero for the next launch (ordered by the kernel boundary)
    if (tid >= f0 && tid < F) {
        double v = 0.0;
        for (int gg = 0; gg < groups; ++gg) v += agent_load(S.group_partial + gg * F + tid);
        if (tid < F - 1) {
            io.summary[tid] = v;
        } else if (io.transitions && v != 0.0) {
            *io.transitions += (uint64_t)v;
        }
    }
    if (tid <= kEpilogueGroups) S.tickets[tid * kTicketStride] = 0u;
}

// Up to n_steps transitions per running env in one launch; state lives in VGPRs between steps, finished envs
// take their next scenario from the ring.
// The shard's kernel (HEADLINE instantiation of rollout_kernel<10>) is compiled for THREE resident waves per SIMD (<= 168
// VGPRs) and uses the compact LDS layout (carve<.., COMPACT>: 12 workgroups per CU); the generic 10-half-plane instantiations are
// left to the register allocator (two waves).
constexpr int kGeom20Waves = 3;
// DYNAMIC SCHEDULE of the shard's kernel (Params::sched == kSchedDynamic; round 5).  The static 3-of-4 schedule needs every
// workgroup of a sub-launch resident in ONE round: a single slot held by somebody else — a scenario-generator workgroup of the
// asynchronous fill that runs for milliseconds — sends a step workgroup to a second round and doubles the sub-launch.  Here the
// grid is a set of PERSISTENT workgroups (at most the resident slots) that take (env, visit)
// items from a device queue: a call of n steps is V = Params::dyn_visits visits of n / V steps per env, queued visit-major (all
// envs' visit 0, then all visit 1, ...), so the chip is busy for V B / G "rounds" of n / V steps whatever G is, with no launch
// boundary (and no slowest-wave tail) in between; short visits (~56 steps) also even out the envs that sit in a jam.  An env's
// visits must run in order: a workgroup that takes visit k of an env waits until dyn_queue[1 + env] == k (release / acquire at agent scope around the env's state in HBM).  No deadlock: an
// item's predecessor was dequeued earlier, i.e. is held by a workgroup that is running.
constexpr int kSchedDynamic = 100;
template <int MAXL, bool UNI, bool HEADLINE = false, bool KD = false>
__global__ __launch_bounds__(kMaxBlock, (MAXL == 10 && HEADLINE ? kGeom20Waves : 1)) void rollout_kernel(Params P_in, const StateView* Sd, const int* ring_filled_in,
                                                            RolloutView R, int n_steps, const double* ext_action) {
#include "rollout_body.inc"
}

// cn_rollout_trace: the generic rollout_kernel<MAXL, false, false, KD> (an ORCA robot is holonomic) with the per-step rows of T
// written on the way — the same body (rollout_body.inc) with its CN_ROLLOUT_TRACE stores: at the top of a step the state BEFORE
// the transition (every agent lane of a running env: its eight AgentRegs doubles as four 16-byte stores) and the robot lane's
// episode ordinal and step index, behind step_core what the transition returned.  Whatever the geometry, a traced call runs
// this kernel: never the fused one, never the shard's.
template <int MAXL, bool KD>
__global__ __launch_bounds__(kMaxBlock, 1) void rollout_trace_kernel(Params P_in, const StateView* Sd, const int* ring_filled_in,
                                                                     RolloutView R, int n_steps, const cn_trace_out T) {
    constexpr bool UNI = false, HEADLINE = false;
    const double* const ext_action = nullptr;
#define CN_ROLLOUT_TRACE
#include "rollout_body.inc"
#undef CN_ROLLOUT_TRACE
}

// cn_rollout_actions: the generic rollout_kernel<MAXL, UNI, false, KD> of an external robot with the call's action table
// (double [B][n_steps][2]) in place of the one action block every step of a launch shares — the same body under
// CN_ROLLOUT_ACTIONS, which moves ext_action to the step's row before step_core reads it.  n_steps cn_rollout_step launches
// as one.  rollout_actions_trace_kernel is the same with the CN_ROLLOUT_TRACE stores (out != NULL): two kernels rather than
// one that tests T's pointers, so that an untraced call — a planner's — holds no trace registers across the step loop.
template <int MAXL, bool UNI, bool KD>
__global__ __launch_bounds__(kMaxBlock, 1) void rollout_actions_kernel(Params P_in, const StateView* Sd, const int* ring_filled_in,
                                                                       RolloutView R, int n_steps, const double* action_table) {
    constexpr bool HEADLINE = false;
#define CN_ROLLOUT_ACTIONS
#include "rollout_body.inc"
#undef CN_ROLLOUT_ACTIONS
}

template <int MAXL, bool UNI, bool KD>
__global__ __launch_bounds__(kMaxBlock, 1) void rollout_actions_trace_kernel(Params P_in, const StateView* Sd,
                                                                             const int* ring_filled_in, RolloutView R, int n_steps,
                                                                             const double* action_table, const cn_trace_out T) {
    constexpr bool HEADLINE = false;
#define CN_ROLLOUT_ACTIONS
#define CN_ROLLOUT_TRACE
#include "rollout_body.inc"
#undef CN_ROLLOUT_TRACE
#undef CN_ROLLOUT_ACTIONS
}

// cn_lookahead_actions: rollout_actions_kernel over B K VIRTUAL envs — branch (b, k) is virtual env v = b K + k, P_in.B = B K,
// action_table double [B K][n_steps][2] — that start from the state of env v / K as it stands and leave the engine as it was.
// The same body under CN_ROLLOUT_LOOKAHEAD: every load of the prologue goes through the source env; the book starts fresh;
// an ended branch stops stepping and nothing takes its place (no ring, no record, no io block: R.io is NULL); the tail stores
// the branch's outputs through Od, a device copy of the caller's cn_lookahead_out, and nothing else.
template <int MAXL, bool UNI, bool KD>
__global__ __launch_bounds__(kMaxBlock, 1) void rollout_lookahead_kernel(Params P_in, const StateView* Sd, RolloutView R, int n_steps,
                                                                         const double* action_table, const cn_lookahead_out* Od,
                                                                         int n_candidates) {
    constexpr bool HEADLINE = false, GOAL = false;
#define CN_ROLLOUT_ACTIONS
#define CN_ROLLOUT_LOOKAHEAD
#include "rollout_body.inc"
#undef CN_ROLLOUT_LOOKAHEAD
#undef CN_ROLLOUT_ACTIONS
}

// Its goal form (cn_lookahead_set_goal_weight with a weight != 0): the same body under GOAL = true.  A kernel of its own, so
// that the one above keeps its instructions; the same arguments, with the engine's weight as one double behind *Od (the tail
// reads it there: rollout_body.inc says why it is not an argument here as it is for the lane-per-branch kernels).
template <int MAXL, bool UNI, bool KD>
__global__ __launch_bounds__(kMaxBlock, 1) void rollout_lookahead_goal_kernel(Params P_in, const StateView* Sd, RolloutView R,
                                                                              int n_steps, const double* action_table,
                                                                              const cn_lookahead_out* Od, int n_candidates) {
    constexpr bool HEADLINE = false, GOAL = true;
#define CN_ROLLOUT_ACTIONS
#define CN_ROLLOUT_LOOKAHEAD
#include "rollout_body.inc"
#undef CN_ROLLOUT_LOOKAHEAD
#undef CN_ROLLOUT_ACTIONS
}

}  // namespace cn
