// Device side of the scenario ring: the generators' entry kernels (reset, rollout begin), the ring's rules — which ordinal
// lives in which slot, who may claim and publish one — every fill kernel, the scenario cache of the wave generators, and what a
// transition kernel asks of the ring (scenario_ready, load_from_ring).  The host side is scenario_ring_host.h; when a fill runs
// is fill_plan.h.  Part of the env translation unit (crowdnav_amd.hip) only: the value-network unit includes step_kernels.h alone.
#pragma once
#include "step_kernels.h"

namespace cn {

// Lane-per-scenario generation: try the register-only head generator first (no memory traffic), redo the scenario
// with the memory-backed one (word-major HBM scratch: any number of waves per CU) in the rare case its 227 words do not
// suffice.  Returns random() calls consumed.
__device__ __forceinline__ uint64_t generate_scenario_lane(const ScenarioCfg& C, uint32_t seed, size_t base,
                                                           double2* pos, double2* vel, double2* goal, double2* rv,
                                                           uint32_t* hbm_column, int hbm_stride, bool keep_state,
                                                           int* pos_out) {
    if (!keep_state) {
        Mt19937Head head;
        const uint64_t n = generate_scenario(C, head, seed, base, pos, vel, goal, rv);
        if (!head.dead()) return n;
    }
    Mt19937 rng{hbm_column, hbm_stride, 0};
    const uint64_t n = generate_scenario(C, rng, seed, base, pos, vel, goal, rv);
    if (keep_state && pos_out) *pos_out = rng.pos;
    return n;
}

// New episode of env b: new Human objects, new ORCA policies, new rvo2 simulators (the robot's persists) — their kd-tree orders
// start as the identity.  Lanes first, first + stride, ... of kd_valid[1..A): (1, 1) from a kernel with one lane per env,
// (1 + threadIdx.x, blockDim.x) from one with a workgroup per env.
__device__ __forceinline__ void clear_human_sims(const Params& P, const StateView& S, int b, int first, int stride) {
    if (P.kd)
        for (int a = first; a < P.A; a += stride) S.kd_valid[(size_t)b * P.A + a] = 0;
}

// np.random.seed(seed) + scenario of one env per lane (lane = env)
__global__ __launch_bounds__(kWave) void reset_kernel(Params P, ScenarioCfg C, StateView S, const uint32_t* seeds,
                                                     const uint8_t* mask, uint64_t* draws) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    if (mask && !mask[b]) return;
    const uint64_t n = generate_scenario_lane(C, seeds[b], (size_t)b * P.A, S.pos, S.vel, S.goal, S.rv,
                                                      S.mt_key + b, P.B, true, &S.mt_pos[b]);
    S.gtime[b] = 0.0;
    S.theta[b] = 1.5707963267948966;  // robot.set(..., np.pi / 2)
    if (draws) draws[b] = n;
    clear_human_sims(P, S, b, 1, 1);
}

__global__ void mt_probe_kernel(uint32_t* key, uint32_t seed, int n, double* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Mt19937 rng{key, 1, 0};
    rng.seed(seed);
    for (int i = 0; i < n; ++i) out[i] = rng.random();
}

// Rollout bookkeeping lives behind ONE pointer to a device copy of the caller's cn_rollout_io: the ~20
// pointers in it are needed only when an episode ends, and keeping them out of the kernel arguments keeps
// them out of the SGPR file of the step loop.
struct RolloutView {
    const cn_rollout_io* io;
    const double* discount;  // [discount_len]
    int discount_len;
};

// io.active[] states
enum { kRetired = 0, kRunning = 1, kWaitingScenario = 2 };

__device__ __forceinline__ int64_t episode_id(const cn_rollout_io& io, int b, int ordinal) {
    return io.env_offset + b + (int64_t)ordinal * io.env_stride;
}
__device__ __forceinline__ uint32_t episode_seed(const cn_rollout_io& io, int64_t c) {
    return io.seed_base + (uint32_t)((uint64_t)c % io.seed_mod);
}

// ---- the rules of the scenario ring, each stated once ------------------------------------------------------------
// the episode limit of a rollout (io.episode_limit < 0: none): episode c is not run
__device__ __forceinline__ bool past_episode_limit(const cn_rollout_io& io, int64_t c) {
    return io.episode_limit >= 0 && c >= io.episode_limit;
}
// first ordinal the rollout may still ask for (an env waiting for a scenario has not consumed ep_count yet).  A fill that
// runs BESIDE a transition kernel takes both arguments from one load of StateView::ep_word — (state, episodes finished) of the
// env as ONE word, stored once by the transition kernel when it ends: two separate loads of io->active / io->ep_count could
// pair an old state with a new count and claim a slot whose scenario has not been consumed yet
__device__ __forceinline__ int ring_next_ordinal(int ep_count, int state) { return ep_count + (state == kWaitingScenario ? 0 : 1); }
// the one ordinal of [next, next + D) that lives in ring slot `slot` (ordinal o lives in slot o % D; D = Params::ring_mod)
__device__ __forceinline__ int ring_slot_ordinal(int next, int slot, int D) { return next + ((slot - next % D) + D) % D; }
// Asynchronous fill: claim slot idx = (env, ordinal % D) for `ordinal`.  False: resident already, or another fill launch is
// generating (or has generated) exactly this scenario.  Only slots whose scenario the env consumed before the transition
// kernel running beside the fill was launched are ever overwritten.
__device__ __forceinline__ bool ring_claim_slot(const StateView& S, int idx, int ordinal) {
    const int want = ordinal + 1;
    const int have = S.ring_claim[idx];
    return have < want && atomicCAS(&S.ring_claim[idx], have, want) == have;
}
// ... and publish it, by the whole workgroup that wrote the scenario: a device-scope release store of ordinal + 1 to
// ring_ready (scenario_ready is the acquire side)
__device__ __forceinline__ void ring_publish_slot(const StateView& S, int idx, int ordinal) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // (a cached copy is written by A lanes, not by lane 0 alone)
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&S.ring_ready[idx], ordinal + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// (re)start bookkeeping of env b, which begins its episode ordinal 0 with nothing in its ring (`on`: it runs at all)
__device__ __forceinline__ void begin_env(const StateView& S, const cn_rollout_io& io, int b, bool on) {
    io.active[b] = on ? kRunning : kRetired;
    S.ep_word[b] = on ? kRunning : kRetired;
    io.ep_count[b] = 0;
    io.cur_steps[b] = 0;
    io.cur_return[b] = 0.0;
    if (io.cur_danger) io.cur_danger[b] = 0;
    if (io.cur_danger_dmin_sum) io.cur_danger_dmin_sum[b] = 0.0;
    S.ring_filled_in[b] = 0;
    S.ring_filled_out[b] = 0;
}

__global__ __launch_bounds__(kWave) void rollout_begin_kernel(Params P, ScenarioCfg C, StateView S, RolloutView R) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const cn_rollout_io io = *R.io;
    const int64_t c0 = episode_id(io, b, 0);
    const bool on = !past_episode_limit(io, c0);
    begin_env(S, io, b, on);
    clear_human_sims(P, S, b, 1, 1);
    if (!on) return;
    generate_scenario_lane(C, episode_seed(io, c0), (size_t)b * P.A, S.pos, S.vel, S.goal, S.rv, S.mt_key + b,
                                   P.B, false, nullptr);
    S.mt_pos[b] = -1;
    S.gtime[b] = 0.0;
}

// Scenario ring fill: one lane per (env, missing scenario) generates an episode that has not been generated yet, so that ordinals [next, next + D) are resident when the rollout
// launch that follows needs them.  The lane runs the register-only head generator; the
// rare scenario whose rejection chain outruns its 227 words is queued in redo_list and regenerated by ring_redo_kernel
// with a memory-backed generator from a small fixed pool (624 x kRedoLanes words, not 624 x B x D).
constexpr int kRedoLanes = 4096;
// ep_snap != NULL (the lagged fill, beside a transition kernel: fill_plan.h): (state, episodes finished) of env b comes from
// ep_snap[b], the copy of StateView::ep_word that ring_fill_begin_kernel took in front of this launch — ONE reading per env
// for all its lanes, whether that env's workgroup of the running launch had stored the word yet or not.
__global__ __launch_bounds__(kWave) void ring_fill_begin_kernel(int B, const int* ep_word, int* ep_snap, int* redo_count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) redo_count[0] = 0, redo_count[1] = 0;
    if (b < B) ep_snap[b] = __hip_atomic_load(&ep_word[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// first_step != 0 (engines whose cn_rollout runs the two-wave kernel): the slot's solved first step (StateView::ring_vel0) dies with
// the scenario it belonged to, and the slot joins the job list of ring_first_step_kernel (rollout_fused.h), which follows on the
// same stream — one atomic per wave, as ring_fill_scan_kernel appends.
__global__ __launch_bounds__(kWave) void ring_fill_kernel(Params P, ScenarioCfg C, StateView S, RolloutView R, const int* ep_snap,
                                                         int first_step) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int D = P.ring_mod;  // slots per env; the fill tops up to next + D and publishes that level
    if (idx >= P.B * D) return;
    // D slots per env (synchronous ring): lane (b, slot), neighbouring lanes write neighbouring slots.  2 D slots (lagged fill):
    // lane (k, b), k-major, the k-th scenario env b is missing — an env misses as many as it has consumed since the previous
    // fill, so the lanes with work are the first rows of this numbering, whole waves of them; numbered by slot the same
    // scenarios sat scattered over twice as many half-empty waves (and, beside a launch, nobody waits for the scattered stores).
    const bool by_slot = D == P.ring_depth;
    const int k = by_slot ? idx % D : idx / P.B, b = by_slot ? idx / D : idx - k * P.B;
    const cn_rollout_io* io = R.io;
    const int state = ep_snap ? ep_snap[b] & 3 : io->active[b];
    const int next = ring_next_ordinal(ep_snap ? ep_snap[b] >> 2 : io->ep_count[b], state);
    if (k == 0) S.ring_filled_out[b] = next + D;
    if (state == kRetired) return;
    const int level = S.ring_filled_in[b];  // (ordinals below the stored level are resident from earlier fills)
    const int ordinal = by_slot ? ring_slot_ordinal(next, k, D) : max(level, next) + k;
    if (ordinal < level || ordinal >= next + D) return;
    const int64_t c = episode_id(*io, b, ordinal);
    if (past_episode_limit(*io, c)) return;
    const uint32_t seed = episode_seed(*io, c);
    const int ring_idx = b * D + ordinal % D;
    if (first_step) {  // (the lanes that are still here: every one of them generates)
        S.ring_vel0_ok[ring_idx] = 0;
        const unsigned long long m = __ballot(1);
        const int lane = threadIdx.x & (kWave - 1), leader = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&S.redo_count[1], __popcll(m));
        base = __shfl(base, leader);
        S.first_list[base + __popcll(m & ((1ull << lane) - 1ull))] = ring_idx;
    }
    Mt19937Head head;
    generate_scenario(C, head, seed, (size_t)ring_idx * P.A, S.ring_pos, nullptr, S.ring_goal, S.ring_rv);
    if (head.dead()) S.redo_list[atomicAdd(S.redo_count, 1)] = make_int2(ring_idx, (int)seed);
}

// The scenarios ring_fill_kernel queued: a fixed grid of kRedoLanes lanes strides over the list, each lane with
// its own column of the word-major generator pool.
__global__ __launch_bounds__(kWave) void ring_redo_kernel(Params P, ScenarioCfg C, StateView S, int first_step) {
    const int lane = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = *S.redo_count;
    for (int k = lane; k < n; k += kRedoLanes) {
        const int2 job = S.redo_list[k];
        if (first_step) S.ring_vel0_ok[job.x] = 0;  // (already on ring_fill_kernel's job list)
        Mt19937 rng{S.ring_mt_key + lane, kRedoLanes, 0};
        generate_scenario(C, rng, (uint32_t)job.y, (size_t)job.x * P.A, S.ring_pos, nullptr, S.ring_goal, S.ring_rv);
    }
}

// ---- wave-cooperative variants (scenario_wave.h): one 64-lane workgroup per scenario -----------------------------
__global__ __launch_bounds__(kWave) void reset_wave_kernel(Params P, ScenarioCfg C, StateView S, const uint32_t* seeds,
                                                          const uint8_t* mask, uint64_t* draws) {
    __shared__ WaveScratch scratch;
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    // the env's own numpy stream continues where the scenario left it (cn_sarl_explore): mt_key [624][B], mt_pos [B]
    const uint64_t n = generate_scenario_wave(C, scratch, seeds[b], (size_t)b * P.A, S.pos, S.vel, S.goal, S.rv, S.mt_key + b,
                                              P.B, &S.mt_pos[b]);
    if (threadIdx.x == 0) {
        S.gtime[b] = 0.0;
        S.theta[b] = 1.5707963267948966;
        if (draws) draws[b] = n;
    }
    clear_human_sims(P, S, b, 1 + threadIdx.x, blockDim.x);
}

__global__ __launch_bounds__(kWave) void rollout_begin_wave_kernel(Params P, ScenarioCfg C, StateView S, RolloutView R) {
    __shared__ WaveScratchFill scratch;
    const int b = blockIdx.x;
    const cn_rollout_io io = *R.io;
    const int64_t c0 = episode_id(io, b, 0);
    const bool on = !past_episode_limit(io, c0);
    if (threadIdx.x == 0) {
        begin_env(S, io, b, on);
        S.gtime[b] = 0.0;
        S.mt_pos[b] = -1;
    }
    clear_human_sims(P, S, b, 1 + threadIdx.x, blockDim.x);
    if (P.async_fill)
        for (int t = threadIdx.x; t < P.ring_depth; t += blockDim.x) {  // nothing resident, nothing claimed
            S.ring_ready[(size_t)b * P.ring_depth + t] = 0;
            S.ring_claim[(size_t)b * P.ring_depth + t] = 0;
        }
    if (!on) return;
    generate_scenario_wave(C, scratch, episode_seed(io, c0), (size_t)b * P.A, S.pos, S.vel, S.goal, S.rv);
}

// A seeded scenario is a pure function of its seed, and the reference's own evaluation phases replay a fixed set of them
// ('val': 100 cases, 'test': 500; crowd_sim.py:272-283).  With 20 humans on the 4 m circle 60 % of all rejection-sampling
// attempts of the 1021 bench seeds belong to the ten hardest (up to 3.1 M attempts = 118 ms of one wave, each time) — so a
// rollout whose episode seeds come from at most kScenarioCacheMax values keeps every scenario it has generated: the first
// workgroup that needs seed index k generates it into the ring slot and copies it to the cache (release), later ones copy it
// from there (acquire).  Two workgroups may generate the same seed at the same time: they write the same bits.
constexpr int kScenarioCacheMax = 4096;
template <class Scratch>
__device__ __forceinline__ void cached_scenario_wave(const Params& P, const ScenarioCfg& C, const StateView& S, Scratch& scratch,
                                                     const cn_rollout_io& io, int64_t c, size_t base) {
    const int lane = threadIdx.x;
    const bool use = S.cache_n > 0;
    const int k = use ? (int)((uint64_t)c % io.seed_mod) : 0;
    if (use && __hip_atomic_load(&S.cache_state[k], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 1) {
        if (lane < P.A) {
            const size_t ci = (size_t)k * P.A + lane;
            S.ring_pos[base + lane] = S.cache_pos[ci];
            S.ring_goal[base + lane] = S.cache_goal[ci];
            S.ring_rv[base + lane] = S.cache_rv[ci];
        }
        return;
    }
    generate_scenario_wave(C, scratch, episode_seed(io, c), base, S.ring_pos, nullptr, S.ring_goal, S.ring_rv);
    if (!use) return;
    __syncthreads();  // (lane 0 wrote the slot; same workgroup: visible after the barrier)
    if (lane < P.A) {
        const size_t ci = (size_t)k * P.A + lane;
        S.cache_pos[ci] = S.ring_pos[base + lane];
        S.cache_goal[ci] = S.ring_goal[base + lane];
        S.cache_rv[ci] = S.ring_rv[base + lane];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (lane == 0) __hip_atomic_store(&S.cache_state[k], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kWave) void ring_fill_wave_kernel(Params P, ScenarioCfg C, StateView S, RolloutView R) {
    __shared__ WaveScratchFill scratch;
    const int idx = blockIdx.x;  // (env, ring slot)
    const int D = P.ring_depth;
    const int b = idx / D, slot = idx - b * D;
    const cn_rollout_io io = *R.io;
    const int state = io.active[b];
    const int next = ring_next_ordinal(io.ep_count[b], state);
    if (slot == 0 && threadIdx.x == 0) S.ring_filled_out[b] = next + D;
    if (state == kRetired) return;
    const int ordinal = ring_slot_ordinal(next, slot, D);
    if (ordinal < S.ring_filled_in[b]) return;
    const int64_t c = episode_id(io, b, ordinal);
    if (past_episode_limit(io, c)) return;
    cached_scenario_wave(P, C, S, scratch, io, c, ((size_t)b * D + slot) * P.A);
}

// Asynchronous flavour (CN_FLAG_ASYNC_SCENARIO_FILL): runs on a side stream NEXT to the transition kernel, as a WORK LIST.  Two
// launches on the fill stream: ring_fill_scan_kernel examines the (env, urgency) items — urgency u = how many episodes ahead of
// the env's next one the scenario lies — one per lane, claims the slot for the ordinal the env will need there (an earlier fill
// launch may still be working on it: ring_claim_slot) and appends the claimed (env, ordinal) pairs to a job list, URGENCY-MAJOR
// (every env's nearest missing scenario before anybody's far one: a hard scenario — tens of milliseconds of one wave — far
// ahead in the ring has the whole ring's worth of steps to finish); ring_fill_jobs_kernel is a fixed grid of persistent one-wave
// generator workgroups (CROWDNAV_AMD_FILL_QUEUE_WGS) that pop kFillJobBatch jobs at a time, generate them and publish each
// (ring_publish_slot).  No workgroup ever waits for another one.
// (Rounds 2-5 ran one workgroup per (env, slot) instead: 4096 x 144 = 590 k workgroups of which a fifth have something to do cost
// a 999-step call 4.5 ms of dispatch beside its transition kernel.  The figures of both, and of 256 .. 2048 generator
// workgroups, are in profiles/HISTORY.md.)
//   list: int [2 + 2 * B * D]: [0] jobs appended, [1] jobs popped, then the (env, ordinal) pairs; [0] and [1] are zeroed on the
//   fill stream in front of the scan (one list per side stream: fill launches overlap)
__global__ __launch_bounds__(256) void ring_fill_scan_kernel(Params P, StateView S, RolloutView R, int* list) {
    const int D = P.ring_depth;
    const int total = P.B * D;
    const cn_rollout_io* io = R.io;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    const int u = item / P.B, b = item - u * P.B;
    int ordinal = 0;
    bool claimed = false;
    if (item < total) {
        const int word = __hip_atomic_load(&S.ep_word[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (state, episodes finished)
        const int state = word & 3;
        if (state != kRetired) {
            ordinal = ring_next_ordinal(word >> 2, state) + u;
            if (!past_episode_limit(*io, episode_id(*io, b, ordinal))) claimed = ring_claim_slot(S, b * D + ordinal % D, ordinal);
        }
    }
    // one atomic per wave: the wave's claimed items go to consecutive list entries in lane (= env) order
    const unsigned long long m = __ballot(claimed);
    if (m == 0ull) return;
    const int lane = threadIdx.x & (kWave - 1);
    int base = 0;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(&list[0], __popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (claimed) {
        const int k = base + __popcll(m & ((1ull << lane) - 1ull));
        list[2 + 2 * k] = b;
        list[3 + 2 * k] = ordinal;
    }
}

constexpr int kFillJobBatch = 4;  // jobs a generator workgroup pops at a time
__global__ __launch_bounds__(kWave) void ring_fill_jobs_kernel(Params P, ScenarioCfg C, StateView S, RolloutView R, int* list) {
    __shared__ WaveScratchFill scratch;
    const int lane = threadIdx.x;
    const int D = P.ring_depth;
    const cn_rollout_io* io = R.io;
    const int jobs = list[0];  // (complete: the scan kernel ran in front of this one on the same stream)
    int first = 0;
    do {
        if (lane == 0) first = atomicAdd(&list[1], kFillJobBatch);
        first = __shfl(first, 0);
        // lane l < kFillJobBatch holds job first + l; the batch's scenarios are generated one after the other by the whole wave
        int jb = 0, jord = 0;
        const bool have = lane < kFillJobBatch && first + lane < jobs;
        if (have) jb = list[2 + 2 * (first + lane)], jord = list[3 + 2 * (first + lane)];
        unsigned long long todo = __ballot(have);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const int b = __shfl(jb, src), ord = __shfl(jord, src);
            const int idx = b * D + ord % D;
            cached_scenario_wave(P, C, S, scratch, *io, episode_id(*io, b, ord), (size_t)idx * P.A);
            ring_publish_slot(S, idx, ord);
        }
    } while (first + kFillJobBatch < jobs);
}

// Is scenario `ordinal` of env b resident?  Synchronous fill: the launch-time fill level; asynchronous: the slot's own flag
// (acquire at device scope: the scenario data written by the concurrently running fill kernel is visible after it).
__device__ __forceinline__ bool scenario_ready(const Params& P, const StateView& S, int env, int ordinal, int ring_filled) {
    if (!P.async_fill) return ordinal < ring_filled;
    const int* flag = S.ring_ready + (size_t)env * P.ring_depth + ordinal % P.ring_depth;
    return __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == ordinal + 1;
}

__device__ __forceinline__ void load_from_ring(const Params& P, const StateView& S, const Lane& L, int slot,
                                               AgentRegs& r) {
    const size_t ri = ((size_t)L.env * P.ring_mod + slot) * P.A + L.a;
    const double2 p = S.ring_pos[ri], g = S.ring_goal[ri], q = S.ring_rv[ri];
    r.px = p.x, r.py = p.y, r.vx = 0.0, r.vy = 0.0, r.gx = g.x, r.gy = g.y, r.rad = q.x, r.vpref = q.y;
}

}  // namespace cn
