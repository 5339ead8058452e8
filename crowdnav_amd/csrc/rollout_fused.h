// The fused rollout for the small-crowd geometries (<= 5 candidate neighbours per agent, one wave per workgroup,
// holonomic robot): the same transition as step_core (step_kernels.h) / rollout_kernel (rollout_kernels.h) — same functions for every number
// it computes — with FOUR LDS exchange points per step instead of nine:
//
//   [stage]   agent lanes   float32 view of the agents, preferred velocities        (written at the END of the previous step)
//   pairs     pair lanes    the agent's candidate distances in registers (no d2 round trip), rank, half-plane   -> barrier 1
//   cands     (agent, half-plane) lanes   1-D solutions (lp_line_candidate)                                     -> barrier 2
//   solve     agent lanes   scan (+ candidate-form 3-D fallback for the infeasible ones, 3 barriers only then);
//                           the robot's action reaches its env's lanes by a wave shuffle, not through LDS;
//                           float64 swept distance / goal distance                                             -> barrier 3
//   reduce    agent lanes   EVERY lane of an env reduces the env's distances to reward / done / info itself (idle lanes
//                           otherwise), so the episode bookkeeping that decides what the agents do next — advance, load the
//                           next scenario from the ring, pause — needs no flag broadcast; integrate; stage the next step
//                                                                                                                -> barrier 4
// The env's episode bookkeeping (rollout_kernels.h: EpisodeBook — global_time, the return / danger accumulators, episodes
// finished, ring fill level, running / waiting / retired) is replicated on the env's lanes; only the robot lane writes it
// out: records, and the book at the end of the launch.
// Launch conditions (cn_rollout / cn_rollout_step check them, everything else runs rollout_kernel): 5-half-plane
// instantiation, NC <= 5, pairs <= 64, nA * 5 <= 64, 64 threads, holonomic robot.
// SPLIT (further down): the headline geometry's cn_rollout as TWO waves per workgroup — the phases above, dealt to an ORCA
// wave and an env wave that meet at two s_barrier per step.
#pragma once
#include "rollout_kernels.h"

namespace cn {

constexpr int kFusedMaxNC = 5;

// A wave-uniform value pinned in vector registers.  The eight float64 parameters of the step (dt, time limit, rewards,
// discomfort distance / factor, safety space) arrive as kernel arguments in SGPRs; with ~100 SGPRs live in the step loop the
// register allocator spilled that 16-dword block into VGPR lanes and re-read it with v_readlane five times per step (107
// v_readlane of the loop's ~1 450 instructions: every one a VALU issue slot).  As VALU operands they are needed in VGPRs
// anyway; the empty asm makes the copy explicit and opaque, so the values stay there (16 VGPRs; the kernel has room up to 168).
template <typename T>
__device__ __forceinline__ T in_vgpr(T x) {
    asm volatile("" : "+v"(x));
    return x;
}

// What the NEXT step's pair and collide phases read: the float32 view of the agents, float64 position, radii.
// `kin`: where the view goes — Smem::kin, or the env wave's staging rows of the two-wave kernel (split_orca_wave).
__device__ __forceinline__ void stage_agent(const Params& P, const Smem& s, const Lane& L, const AgentRegs& r,
                                            double human_safety, float4* kin) {
    if (L.lane >= P.nA) return;
    kin[L.lane] = make_float4((float)r.px, (float)r.py, (float)r.vx, (float)r.vy);
    s.posd[L.lane] = make_double2(r.px, r.py);
    s.rad[L.lane] = r.rad;
    s.hview[L.lane] = (float)(r.rad + 0.01 + human_safety);
}

// The agent's preferred velocity — towards its goal, unit length once farther than 1 m (orca.py:113-115): a float64 norm and
// two float64 divisions, ~450 clock ticks of dependent latency on 12 lanes — and linearProgram2's start point (Appendix A.4).
// Nothing reads them before the candidates phase, so they are computed INSIDE the pair phase, branch-free on every lane: one
// basic block with the float32 pair arithmetic, and the scheduler interleaves the two dependency chains.
__device__ __forceinline__ void preferred_velocity(const AgentRegs& r, float max_speed, bool solve, float4& sol, float4& start) {
    const double gdx = r.gx - r.px, gdy = r.gy - r.py;
    const double speed = norm2(gdx, gdy);
    const float pref_x = (float)(speed > 1.0 ? gdx / speed : gdx);
    const float pref_y = (float)(speed > 1.0 ? gdy / speed : gdy);
    sol = make_float4(pref_x, pref_y, max_speed, solve ? 1.0f : 0.0f);
    float sx, sy;
    lp_start_point(max_speed, pref_x, pref_y, sx, sy);
    start = make_float4(sx, sy, 0.0f, 0.0f);
}

// The fused kernel is ONE wave per workgroup: LDS instructions of a wave execute in order, so what the phases need between a
// lane's write and another lane's read is only that the compiler keeps the accesses in program order — not s_barrier with
// its s_waitcnt lgkmcnt(0) in front (the LDS queue drained five times per step).
#define CN_FUSED_SYNC() wave_lds_sync()

// Issue priority: a launch ends with its slowest wave, and that is a wave whose env sits in a jam and takes the 3-D fallback
// every step — 1.6 x the latency of a step without it — while the wave it shares the SIMD with has slack.  A wave entering the
// fallback raises its priority (s_setprio 3) and keeps it until the first step that does without (a jam lasts many steps):
// nothing at 20 steps per launch, +3-5 % at 1000.
// The one-pass fallback runs the four planar programs of an infeasible agent on four lanes (orca_device.h: lp3_inner_program /
// lp3_outer_scan); the multi-pass form (more than six infeasible agents in a wave) keeps lp3_scan.

// ---------------------------------------------------------------------------------------------- shared phase bodies
// The one-wave kernel and the two-wave kernel (rollout_fused_split below) run the SAME phase bodies: what differs is which
// wave runs them and what sits between them.

// A pair lane's row: the kin slot of its candidate.  A pair that does not exist (robot invisible to the humans, env beyond
// the batch) points at slot nA = (+inf, +inf): its squared distance is +inf without a select, so the pair phase has no
// data-dependent control flow at all.  The lanes of an agent's candidates are consecutive — (q, 0) .. (q, NC - 1) —
// xbase: the byte address (ds_bpermute: lane * 4) of the group's first lane, (q, 0): lane (q, k) is xbase + 4 k.
struct PairRow {
    int my_info, my_slot, xbase;
};
__device__ __forceinline__ PairRow pair_row_of(const Params& P, const Smem& s, int lane) {
    PairRow pr{0, P.nA, 0};
    if (lane < P.pairs) {
        pr.my_info = s.pinfo[lane];
        const int c = (pr.my_info >> 16) & 0xff;
        pr.xbase = (lane - c) * 4;
        pr.my_slot = ((pr.my_info >> 24) & 1) ? ((pr.my_info >> 8) & 0xff) : P.nA;
    }
    return pr;
}

// The pair's combined radius as its agent's simulator holds it: rview is written in the launch prologue, hview by
// stage_agent — a per-episode constant (the ORCA wave keeps it in a register between episode ends).
__device__ __forceinline__ float pair_rsum(const Smem& s, const PairRow& pr) {
    const int q = pr.my_info & 0xff, ol = (pr.my_info >> 8) & 0xff;
    const float* view = ((pr.my_info >> 25) & 1) ? s.rview : s.hview;
    return view[q] + view[ol];
}

// pairs: candidate distances (Appendix A.2), stable rank = RVO2's sorted-insertion slot, half-plane (A.3).  Pair lanes only.
// `mid` runs between the rank and the stores, in the same basic block (the one-wave kernel's preferred velocity).
// `me`, `other`: kin[q] and kin[my_slot], requested by the caller — the ORCA wave issues them beside its exchange words.
template <typename Mid>
__device__ __forceinline__ void fused_pair_body(const Params& P, const Smem& s, const PairRow& pr, float range_sq, float rsum,
                                                const float4 me, const float4 other, Mid&& mid) {
    const int my_info = pr.my_info;
    const int q = my_info & 0xff, c = (my_info >> 16) & 0xff;
    const float odx = me.x - other.x, ody = me.y - other.y;
    const float mine = odx * odx + ody * ody;
    // The agent's five candidate distances are the `mine` of the five lanes of its group, (q, 0) .. (q, NC - 1): the same
    // subtraction, products and sum on the same kin rows, fetched by a lane exchange (ds_bpermute_b32, the lane's byte address
    // xbase + 4 k as base + immediate offset) instead of five more kin rows and their arithmetic.  Issued right behind `mine`:
    // make_half_plane below does not depend on the rank and covers the exchange.  Every pair lane executes it and reads
    // lanes of its own group only (all pair lanes); a pair that does not exist has my_slot = nA, so its `mine` is +inf as
    // before; k >= NC (no such lane in the group) is +inf by a select.
    uint32_t vbk[kFusedMaxNC];
#pragma unroll
    for (int k = 0; k < kFusedMaxNC; ++k) {
        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(pr.xbase + 4 * k, (int)__float_as_uint(mine));
        vbk[k] = k < P.NC ? got : 0x7f800000u;
    }
    int rank = 0, within = 0;
    {
        // squared distances are +0 .. +inf: their bit patterns order like the floats, so "v < mine, or v == mine and
        // k < c" is bit 31 of v - (mine + [k < c]) and "v < range" is bit 31 of v - range as 32-bit integers: the sign
        // bits are shifted into two words (v_alignbit_b32) and counted once — no compare through VCC / SGPR pairs, no
        // scalar mask logic, none of the hazard s_nop between them (round 6; the shard's rank loop does the same)
        const uint32_t mb = __float_as_uint(mine), rb = __float_as_uint(range_sq);
        uint32_t before = 0u, inside = 0u;
#pragma unroll
        for (int k = 0; k < kFusedMaxNC; ++k) {
            const uint32_t vb = vbk[k];  // +inf for a pair that does not exist: never in range
            const uint32_t tie = (uint32_t)(k - c) >> 31;           // k < c
            before = __builtin_amdgcn_alignbit(before, vb - mb - tie, 31);
            inside = __builtin_amdgcn_alignbit(inside, vb - rb, 31);
        }
        within = __popc(inside);
        rank = __popc(before & inside);
    }
    mid();
    if (c == 0) s.count[q] = within < P.orca.max_neighbors ? within : P.orca.max_neighbors;
    if (mine < range_sq && rank < P.orca.max_neighbors)
        s.lines[q * kLineStride + rank] =
            make_half_plane(P.orca, me.x, me.y, me.z, me.w, other.x, other.y, other.z, other.w, rsum);
}
template <typename Mid>
__device__ __forceinline__ void fused_pair_phase(const Params& P, const Smem& s, const PairRow& pr, float range_sq, float rsum,
                                                 Mid&& mid) {
    // every LDS request of the phase first, none of them behind a condition
    const float4 me = s.kin[pr.my_info & 0xff];
    const float4 other = s.kin[pr.my_slot];
    fused_pair_body(P, s, pr, range_sq, rsum, me, other, mid);
}

// candidates: lane = (agent, half-plane)
template <int MAXL>
__device__ __forceinline__ void fused_candidates(const Params& P, const Smem& s, int lane) {
    if (lane < P.nA * MAXL) {
        const int q = lane / MAXL, k = lane - q * MAXL;
        const float4 so = s.sol[q];
        const float4* lq = s.lines + q * kLineStride;
        s.cand2[q * kLineStride + k] = lp_line_candidate_pairs5(lq, k, lane, so.z, so.x, so.y);
    }
}

// Barrier of the two-wave kernel (further down): every LDS write of this wave has landed (a wave's LDS operations complete
// in order) before the other wave is released.
__device__ __forceinline__ void split_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One item of the one-pass 3-D fallback: lane = (t, m), the t-th agent of `mask` (its t-th set bit: scalar bit tricks, no LDS
// list) and slot m = i (i - 1) / 2 + j of its projections; the item's half-planes are requested once for both stages.
struct Lp3Item {
    int a, m, i, base;
    bool item;
    float4 li, lj;
    float radius;
};
template <int MAXL>
__device__ __forceinline__ Lp3Item lp3_item_of(const Smem& s, int lane, unsigned long long mask) {
    constexpr int kPairs = MAXL * (MAXL - 1) / 2;
    Lp3Item it;
    const int t = lane / kPairs;
    it.m = lane - t * kPairs;
    it.a = 0;
    unsigned long long rest = mask;
#pragma unroll
    for (int u = 0; u < kWave / kPairs; ++u) {
        const int bit = rest ? __ffsll((long long)rest) - 1 : 0;
        it.a = (u == t) ? bit : it.a;
        rest &= rest - 1ull;
    }
    it.item = lane < (int)__popcll(mask) * kPairs;
    it.i = lp3_program_of(it.m), it.base = it.i * (it.i - 1) / 2;
    const float4* la = s.lines + it.a * kLineStride;
    it.li = la[it.i], it.lj = la[it.m - it.base];
    it.radius = s.sol[it.a].z;
    return it;
}
// The head of the one-pass fallback: the item's projection (lp3_project) into the agent's proj row, then the 1-D solution of
// its projected line against the earlier ones of program i into the cand3 row.  Reads only the agent's half-planes and
// sol[a].z — both complete once the pair phase is — so in the two-wave kernel EITHER wave can run it (split_has_head).
template <int MAXL>
__device__ __forceinline__ void lp3_head(const Smem& s, const Lp3Item& it) {
    const float4 pr = lp3_project(it.li, it.lj);
    if (it.item) s.proj[it.a * kLineStride + it.m] = pr;
    CN_FUSED_SYNC();
    if (it.item) {
        // (one (projected line, earlier line) pair per item lane + two shuffle rounds instead of these three masked pairs
        // was built and measured neutral in round 6: 1 229.6 / 1 238.8 vs 1 229.9 / 1 233.7 M — profiles/HISTORY.md)
        const float4* pa = s.proj + it.a * kLineStride + it.base;
        s.cand3[it.a * kLineStride + it.m] =
            lp_line_candidate<MAXL - 2>(pa[it.m - it.base], pa, it.m - it.base, it.radius, -it.li.w, it.li.z, true);
    }
}

// The barrier-3 rule of the two-wave kernel, stated ONCE for both waves: an iteration has a third split_barrier exactly when
// this holds.  `pred` is the prediction word (the agents that were infeasible one step ago), which both waves read from LDS
// after barrier 1 of the iteration, and `u` the step counter both keep identically — so the two waves cannot disagree.  The
// agents of pred must fit the one-pass item layout; the iteration in which the ORCA wave leaves its loop (u == n_steps)
// computes nothing.
template <int MAXL>
__device__ __forceinline__ bool split_has_head(unsigned int pred, int u, int n_steps) {
    return pred != 0u && __popc(pred) * (MAXL * (MAXL - 1) / 2) <= kWave && u < n_steps;
}

// solve: the planar scan, then the candidate-form 3-D fallback for the infeasible agents (wave-uniform branch).  Agent
// lanes with `solve` leave their new velocity in (rx, ry), every other lane (0, 0).  Returns the ballot of the infeasible
// agents (non-zero: the wave took the fallback).
// BASE_PRIO: the issue priority a wave goes back to on its first step without the fallback.
// Two-wave kernel, ORCA wave: `after_scan` runs behind the planar scan (barrier 3 of an iteration that has one) and `have`
// are the agents whose fallback head (lp3_head) the env wave has left in proj / cand3 by then: when every infeasible agent is
// among them the fallback starts at the inner programs.  Otherwise the full path runs — behind barrier 3 the env wave no
// longer writes those rows.
struct NoOp {
    __device__ __forceinline__ void operator()() const {}
};
template <int MAXL, int BASE_PRIO = 0, typename AfterScan = NoOp>
__device__ __forceinline__ unsigned long long fused_solve(const Params& P, const Smem& s, int lane, bool solve, float& rx,
                                                          float& ry, PhaseClock* clk, unsigned long long have = 0ull,
                                                          AfterScan&& after_scan = NoOp{}) {
    (void)P, (void)clk;
    rx = 0.0f, ry = 0.0f;
    int n = 0, fail = 0;
    if (solve) {
        n = s.count[lane];
        const float4 start = s.res[lane];
        rx = start.x, ry = start.y;
        fail = lp_planar_scan<MAXL>(s.lines + lane * kLineStride, s.cand2 + lane * kLineStride, n, rx, ry);
    }
    CN_TICK(clk, 3);
    const bool need = solve && fail < n;
    const unsigned long long nm = __ballot(need);
#ifdef CN_PHASE_TIMING
    if (clk) clk->acc[9] += __popcll(nm);
#endif
    after_scan();
    if (nm == 0ull) __builtin_amdgcn_s_setprio(BASE_PRIO);
    if (nm != 0ull) {  // wave-uniform: some agent of this wave was infeasible
        __builtin_amdgcn_s_setprio(3);
        constexpr int kPairs = MAXL * (MAXL - 1) / 2;
        const int n_todo = __popcll(nm);
        bool one_pass_done = false;  // (wave-uniform)
        if (n_todo * kPairs <= kWave) {
            // one pass: item = lane = (t, m)
            const Lp3Item it = lp3_item_of<MAXL>(s, lane, nm);
            const bool item = it.item;
            const int a = it.a, i = it.i, m = it.m, base = it.base;
            const float4 li = it.li;
            const float radius = it.radius;
            const bool hit = (nm & ~have) == 0ull;  // every infeasible agent's head is there already
            if (!hit) {
                lp3_head<MAXL>(s, it);
                CN_FUSED_SYNC();
            }
            // the four planar programs of an infeasible agent side by side: the item lane of slot (i, 0) runs program i
            // and leaves its solution in the agent's cand2 row (free since the planar scan above), slot i
            if (item && m == base)
                s.cand2[a * kLineStride + i] = lp3_inner_program(s.proj + a * kLineStride, s.cand3 + a * kLineStride, i, li, radius);
            CN_FUSED_SYNC();
            if (need)
                lp3_outer_scan(s.lines + lane * kLineStride, s.cand2 + lane * kLineStride, n, fail, s.sol[lane].z, rx, ry);
            one_pass_done = true;
        } else {
            if (need) s.todo[__popcll(nm & ((1ull << lane) - 1ull))] = lane;
            CN_FUSED_SYNC();
            const int items = n_todo * kPairs;
            for (int p = lane; p < items; p += kWave) {  // projections: lane = (agent, i, j)
                const int t = p / kPairs, m = p - t * kPairs;
                const int a = s.todo[t];
                const int i = lp3_program_of(m), j = m - i * (i - 1) / 2;
                const float4* la = s.lines + a * kLineStride;
                s.proj[a * kLineStride + m] = lp3_project(la[i], la[j]);
            }
            CN_FUSED_SYNC();
            for (int p = lane; p < items; p += kWave) {  // their candidates: lane = (agent, i, k)
                const int t = p / kPairs, m = p - t * kPairs;
                const int a = s.todo[t];
                const int i = lp3_program_of(m), base = i * (i - 1) / 2;
                const float4 li = s.lines[a * kLineStride + i];
                const float4* pa = s.proj + a * kLineStride + base;
                s.cand3[a * kLineStride + m] = lp_line_candidate<MAXL - 2>(pa[m - base], pa, m - base, s.sol[a].z, -li.w, li.z, true);
            }
            CN_FUSED_SYNC();
        }
        if (need && !one_pass_done)
            lp3_scan(s.lines + lane * kLineStride, s.proj + lane * kLineStride, s.cand3 + lane * kLineStride, n,
                     fail, s.sol[lane].z, rx, ry);
    }
    return nm;
}

// The eight float64 parameters of a step, pinned in vector registers (in_vgpr).
struct StepConsts {
    double dt, limit, limit1, success, collision, ddist, dfactor, hsafety;
};
__device__ __forceinline__ StepConsts step_consts(const Params& P) {
    StepConsts K;
    K.dt = in_vgpr(P.dt), K.limit = in_vgpr(P.time_limit), K.limit1 = in_vgpr(P.time_limit - 1.0);
    K.success = in_vgpr(P.success_reward), K.collision = in_vgpr(P.collision_penalty);
    K.ddist = in_vgpr(P.discomfort_dist), K.dfactor = in_vgpr(P.discomfort_factor);
    K.hsafety = in_vgpr(P.human_safety);
    return K;
}

// One float64 distance per agent lane (crowd_sim.py:331-351 for a human, :364-366 for the robot): a human's closest approach
// to the robot during the step, boundary to boundary; the robot's distance to its goal at the end of the step.
//   r: the agent at the START of the step; rp: the robot's position then; act: the robot's new velocity; new_v: this agent's
__device__ __forceinline__ double swept_distance(const AgentRegs& r, bool human, double2 rp, double act_x, double act_y,
                                                 double new_vx, double new_vy, double dt, double robot_rad) {
    const double x1 = r.px - rp.x, y1 = r.py - rp.y;
    const double wx = r.vx - act_x, wy = r.vy - act_y;
    const double2 cp = closest_point(x1, y1, wx, wy, dt);
    const double endx = r.px + new_vx * dt, endy = r.py + new_vy * dt;
    const double d = norm2(human ? cp.x : endx - r.gx, human ? cp.y : endy - r.gy);
    return human ? d - r.rad - robot_rad : d;
}

// reduce (every lane of the env, identically): the env's distances (Smem::closest) to reward / done / info.
// (transition.h states the rule — scan_dmin / scan_collision / outcome_of; this is its branch-free form, kept as text)
struct StepOutcome {
    double reward, dmin;
    int info;
    bool done;
};
__device__ __forceinline__ StepOutcome reduce_env(const Params& P, const Smem& s, int ebase, double gtime, const StepConsts& K) {
    // LDS requests first: the env's distances, the robot's radius
    const double goal_dist = s.closest[ebase];
    const double robot_rad = s.rad[ebase];
    // the reference stops scanning at the first colliding human (dmin keeps the minimum seen before it)
    double dmin = std::numeric_limits<double>::infinity();
    bool collision = false;
    for (int i = 1; i < P.A; ++i) {
        const double c = s.closest[ebase + i];
        const bool hit = c < 0.0;
        dmin = (!collision & !hit & (c < dmin)) ? c : dmin;
        collision = collision | hit;
    }
    // crowd_sim.py:364-389 as a priority chain of selects (timeout > collision > goal > danger > nothing): the
    // same values as the if / elif ladder without its nested branches
    const bool timeout = gtime >= K.limit1;
    const bool reaching = goal_dist < robot_rad;
    const bool danger = dmin < K.ddist;
    double reward = danger ? (dmin - K.ddist) * K.dfactor * K.dt : 0.0;
    int info = danger ? CN_DANGER : CN_NOTHING;
    reward = reaching ? K.success : reward, info = reaching ? CN_REACH_GOAL : info;
    reward = collision ? K.collision : reward, info = collision ? CN_COLLISION : info;
    reward = timeout ? 0.0 : reward, info = timeout ? CN_TIMEOUT : info;
    const bool done = timeout | collision | reaching;
    return StepOutcome{reward, dmin, info, done};
}

// reduce -> account -> episode end of a transition run on every lane of a running env identically (the book is carried
// redundantly; the robot lane writes the record), with the shared statements of rollout_kernels.h: CN_BOOK_TRANSITION, and at an
// episode end CN_END_EPISODE, whose decision is ep.state (kRunning: load ring slot ep.ep_count % P.ring_mod).  The one-wave
// step loop and the env wave each spell the dozen lines around them themselves: the one-wave loop integrates between the
// reduce and the accounting, the env wave requests the next scenario before the record stores, and as ONE helper — function
// or macro — that sequence cost the one-wave kernels 1.1 % (profiles/episode_book_refactor.txt).

// CN_WAVE_TRACE (profiling builds): every wave leaves four 100 MHz timestamps (kernel entry, step loop entry / exit, kernel
// exit) and how many of its steps took the 3-D fallback / ended an episode: scripts/probes/wave_trace.py
#ifdef CN_WAVE_TRACE
static __device__ unsigned long long cn_wave_trace[8192 * 6];
#endif

// ---------------------------------------------------------------------------------------------- the two-wave kernel
// SPLIT: the headline geometry as a workgroup of TWO waves serving the same 2 envs.
//   env wave  (threads 0-63)    everything float64: AgentRegs / EpisodeBook, preferred velocity + start point, swept
//                               distance, reduce / reward / done, integrate, accumulators, records, scenario loads; the launch
//                               prologue and epilogue are the one-wave kernel's own code
//   ORCA wave (threads 64-127)  pairs, candidates, planar scan, 3-D fallback; it carries the float64 positions only to form
//                               the next float32 view with the same `px + vx * dt` as the env wave
// The waves meet at two s_barrier per step.  Iteration of the loop, u = the step whose velocities the ORCA wave computes:
//   barrier 1   both read what the other left: the ORCA wave the "episode ended" word, the env wave the velocities of u - 1
//     ORCA wave: pairs(u) on the kin(u) it staged itself             env wave: integrate u - 1, publish sol / res of u
//   barrier 2
//     ORCA wave: candidates, scan (+ fallback) of u, publish vel(u),  env wave: swept distance, reduce, bookkeeping of u - 1
//                stage kin(u + 1) = its positions + vel(u) dt
// Both sides of an iteration ASSUME that step u - 1 ended no episode.  When it did, the env wave (which now holds the state
// after the episode end: next scenario loaded, env paused or retired) re-stages posd / rad / hview of its lanes, leaves the
// true float32 view in rows of its own (Smem::d2 — kin belongs to the ORCA wave in that window) and posts the word; at
// barrier 1 the ORCA wave then drops the velocities and the view it has just published — they touched LDS only — copies
// the true rows into kin, re-reads its positions and its per-episode constants and computes step u again, while the env
// wave publishes sol / res of the true state and idles past barrier 2.  One ORCA step is redone per episode end of a
// workgroup that is NOT FRESH (~1 in 21 wave-steps at the headline shape when none is).
// Fresh: every env that ended goes on with a ring scenario whose first step was solved when the slot was filled
// (ring_first_step_kernel at the end of this file; StateView::ring_vel0, loaded with the scenario) and the launch has a step left.
// Then step u of the new episode IS solved: the env wave stages the state behind it for the restarted envs' lanes (posd = p0 +
// v0 dt, the d2 row with v0), keeps v0 in a row of its own and posts the envs' bits (bit 1 + el, bit 0 clear).  The ORCA wave
// adopts positions and kin rows of those lanes — the same extra trip — and goes on with step u + 1; the env wave integrates
// step u of those lanes from its v0 row, of the other env from vel as ever.  No iteration is redone, the other env is not
// disturbed, and both waves still count u from the same word.
// The step counters, the discount index and every store to global memory live in the env wave.
// What the waves exchange lives in arrays of the LDS layout that the fused kernels do not otherwise use: Smem::act (the
// published velocities, as float2), Smem::flag[0] (the word) and, with ASSIST, Smem::flag[1] (the prediction word: an
// iteration whose prediction word is non-zero has a third barrier, between the ORCA wave's planar scan and its fallback).
// Issue priority: the ORCA wave is the critical path of a step, the env wave has slack in both windows, and four waves share
// a SIMD — so the ORCA wave runs at priority 1 where the env wave stays at 0 (measured: 1 380 -> 1 473 M env-steps/s at
// 4096 envs x 1000 steps); a jammed wave's 3 during the fallback stands above both.
constexpr int kSplitOrcaPrio = 1;
// ASSIST (CROWDNAV_AMD_SPLIT_ASSIST, cn_create): work of the ORCA wave's chain that the env wave's slack absorbs.
//   kAssistHead  the head of the one-pass 3-D fallback (lp3_head) for the agents that were infeasible ONE STEP AGO — jams
//                persist: that predicts every agent of ~3 in 4 fallback steps.  The ORCA wave leaves its ballot of infeasible
//                agents in Smem::flag[1] beside the velocities; in an iteration whose word is non-zero (split_has_head) the env
//                wave runs the head right behind barrier 2, while the ORCA wave still has candidates and the planar scan in
//                front of it, and the waves meet at a THIRD barrier behind the planar scan.  A hit (every infeasible agent was
//                predicted) starts the ORCA wave's fallback at the inner programs; a miss runs the whole fallback as before
//                (the env wave's rows are overwritten with the same values); a false alarm costs the barrier.
//                The word is stale after an episode end and 0 at launch start: it is a prediction, never a result.
constexpr int kAssistHead = 1;
// the env wave's issue priority while it runs the head: the ORCA wave will wait for it behind its planar scan
#ifndef CN_SPLIT_HEAD_PRIO
#define CN_SPLIT_HEAD_PRIO 2
#endif
// ... and for the rest of window 2 of such an iteration (its float64 work starts late)
#ifndef CN_SPLIT_HEAD_TAIL_PRIO
#define CN_SPLIT_HEAD_TAIL_PRIO 1
#endif

// CN_SPLIT_PROBE (profiling builds; keeps the two-wave route): per launch, summed over the workgroups — iterations, redone
// iterations, fallback steps, iterations with the third barrier, head hits / misses / false alarms, and the shader-clock
// ticks (__builtin_readcyclecounter) each wave waited at barriers 1 / 2 / 3.  The wait at barrier 1 — where window 2 of the
// PREVIOUS iteration ends — is also booked by what that iteration was: one whose step took the fallback (the ORCA wave's
// ballot, which the probe build publishes in Smem::flag[1] whatever ASSIST is), one that had the third barrier.
// scripts/probes/split_probe.py
#ifdef CN_SPLIT_PROBE
constexpr bool kSplitProbe = true;
static __device__ unsigned long long cn_split_probe[32];
#define SPLIT_PROBE_DECL()                                                                                   \
    unsigned long long sp_cnt[7] = {}, sp_wait[3] = {}, sp_w1[2] = {}, sp_n1[2] = {}, sp_dt = 0ull; \
    bool sp_prev_head = false
#define SPLIT_PROBE_WAIT(k, barrier)                                   \
    do {                                                               \
        const unsigned long long sp_t0 = __builtin_readcyclecounter(); \
        barrier;                                                       \
        sp_dt = __builtin_readcyclecounter() - sp_t0;                  \
        sp_wait[k] += sp_dt;                                           \
    } while (0)
// behind barrier 1: `word` = the ballot of the previous iteration's infeasible agents; `head`: has THIS iteration the third barrier
#define SPLIT_PROBE_AFTER_1(word, head)                               \
    do {                                                               \
        if ((word) != 0u) sp_w1[0] += sp_dt, ++sp_n1[0];               \
        if (sp_prev_head) sp_w1[1] += sp_dt, ++sp_n1[1];               \
        sp_prev_head = (head);                                         \
    } while (0)
#define SPLIT_PROBE_STEP(ended, nm, head, pred)                                  \
    do {                                                                         \
        const bool sp_hit = (head) && (nm) != 0ull && ((nm) & ~(unsigned long long)(pred)) == 0ull; \
        ++sp_cnt[0], sp_cnt[1] += (ended) ? 1 : 0, sp_cnt[2] += (nm) != 0ull ? 1 : 0, sp_cnt[3] += (head) ? 1 : 0; \
        sp_cnt[4] += sp_hit ? 1 : 0, sp_cnt[5] += ((nm) != 0ull && !sp_hit) ? 1 : 0, sp_cnt[6] += ((head) && (nm) == 0ull) ? 1 : 0; \
    } while (0)
// cn_split_probe: [0..6] the ORCA wave's counters; [7..9] / [10..12] the ORCA / env wave's waits at barriers 1 / 2 / 3;
// [13 + 4 w ..]: wave w's (0 ORCA, 1 env) barrier-1 waits behind {fallback, third-barrier} iterations, then how many
#define SPLIT_PROBE_FLUSH(lane, base)                                                        \
    do {                                                                                     \
        if ((lane) == 0) {                                                                   \
            if ((base) == 0)                                                                 \
                for (int k = 0; k < 7; ++k) atomicAdd(&cn_split_probe[k], sp_cnt[k]);        \
            for (int k = 0; k < 3; ++k) atomicAdd(&cn_split_probe[((base) ? 10 : 7) + k], sp_wait[k]); \
            for (int k = 0; k < 2; ++k) {                                                    \
                atomicAdd(&cn_split_probe[((base) ? 17 : 13) + k], sp_w1[k]);                \
                atomicAdd(&cn_split_probe[((base) ? 19 : 15) + k], sp_n1[k]);                \
            }                                                                                \
        }                                                                                    \
    } while (0)
#else
constexpr bool kSplitProbe = false;
#define SPLIT_PROBE_DECL() (void)0
#define SPLIT_PROBE_WAIT(k, barrier) barrier
#define SPLIT_PROBE_AFTER_1(word, head) (void)0
#define SPLIT_PROBE_STEP(ended, nm, head, pred) (void)0
#define SPLIT_PROBE_FLUSH(lane, base) (void)0
#endif

template <int MAXL, int ASSIST>
__device__ __forceinline__ void split_orca_wave(const Params& P, const Smem& s, int n_steps) {
    const int lane = (int)threadIdx.x - kWave;
    float2* const vel = reinterpret_cast<float2*>(s.act);
    const float range_sq = P.orca.neighbor_dist * P.orca.neighbor_dist;
    const double c_dt = in_vgpr(P.dt);
    split_barrier();  // the env wave's prologue: pinfo, rview, the staged state of step 0, word = 1
    __builtin_amdgcn_s_setprio(kSplitOrcaPrio);
    const PairRow pr = pair_row_of(P, s, lane);
    double px = 0.0, py = 0.0;
    float rx = 0.0f, ry = 0.0f;
    bool solved = false;
    // Per-episode constants, refreshed in an iteration with `staged` (redo or adopt; the launch's first has it: word = 1).  rsum: rview is
    // written in the prologue only, hview by stage_agent — prologue and episode end.  solved: sol[].w is the env wave's
    // `running && (human || robot_orca)`, and ep.state changes in CN_END_EPISODE alone (next scenario, pause, retire: all
    // under `done`, which sets `ended`); scenario_ready outside of it is the prologue's.
    float rsum = 0.0f;
    const int pq = pr.my_info & 0xff;  // (0 / nA beyond the pair lanes: in bounds)
    SPLIT_PROBE_DECL();
    for (int u = 0;;) {
        SPLIT_PROBE_WAIT(0, split_barrier());  // 1
        // kin(u) was staged at the end of the previous iteration: the pair rows are requested beside the two words
        const int2 words = make_int2(s.flag[0], ((ASSIST & kAssistHead) || kSplitProbe) ? s.flag[1] : 0);
        float4 me = s.kin[pq], other = s.kin[pr.my_slot];
        // the word: bit 0 = redo (below); otherwise bit 1 + el = env el of the workgroup starts its episode from a first step
        // solved at fill time: its lanes ADOPT the state behind that step and nothing is dropped
        const int word = __builtin_amdgcn_readfirstlane(words.x);
        const bool ended = (word & 1) != 0;
        const unsigned int pred = ((ASSIST & kAssistHead) || kSplitProbe) ? (unsigned int)__builtin_amdgcn_readfirstlane(words.y) : 0u;
        if (!ended) ++u;
        if (u >= n_steps) {  // the env wave finishes step n_steps - 1 alone
            split_barrier();  // 2
            break;
        }
        const bool head = (ASSIST & kAssistHead) ? split_has_head<MAXL>(pred, u, n_steps) : false;
        SPLIT_PROBE_AFTER_1(pred, head);
        const bool staged = word != 0;  // (wave-uniform)
        if (staged) {  // the env wave staged the true state (its kin rows in d2: this wave owns kin in window 2): the one extra trip
            // redo: every lane; adopt: the lanes of the adopting envs — the other env's rows and positions are this wave's own
            if (lane < P.nA && (ended || ((word >> (1 + lane / P.A)) & 1) != 0)) {
                const double2 p = s.posd[lane];
                px = p.x, py = p.y;
                s.kin[lane] = reinterpret_cast<const float4*>(s.d2)[lane];
            }
            CN_FUSED_SYNC();
            me = s.kin[pq], other = s.kin[pr.my_slot];
        }
        if (staged) rsum = pair_rsum(s, pr);
        if (lane < P.pairs) fused_pair_body(P, s, pr, range_sq, rsum, me, other, [] {});
        SPLIT_PROBE_WAIT(1, split_barrier());  // 2: sol / res of step u
        fused_candidates<MAXL>(P, s, lane);
        CN_FUSED_SYNC();
        if (staged) solved = lane < P.nA && s.sol[lane < P.nA ? lane : 0].w != 0.0f;
        const unsigned long long nm = fused_solve<MAXL, kSplitOrcaPrio>(P, s, lane, solved, rx, ry, nullptr, head ? pred : 0u, [&] {
            if (head) SPLIT_PROBE_WAIT(2, split_barrier());  // 3: the env wave's proj / cand3 rows of the agents of pred
        });
        if (lane < P.nA) vel[lane] = make_float2(rx, ry);
        if (((ASSIST & kAssistHead) || kSplitProbe) && lane == 0) s.flag[1] = (int)nm;  // the next iteration's prediction word
        // the view of step u + 1, ahead of barrier 1: Agent.step (agent.py:127-135), as the env wave does it.  Nobody reads kin
        // in this window; an episode end found meanwhile drops it (`ended` above)
        if (solved) {
            px = px + (double)rx * c_dt;
            py = py + (double)ry * c_dt;
            s.kin[lane] = make_float4((float)px, (float)py, rx, ry);
        }
        SPLIT_PROBE_STEP(ended, nm, head, pred);
    }
    SPLIT_PROBE_FLUSH(lane, 0);
}

template <bool HEADLINE, bool SPLIT = false, int ASSIST = 0>
// (the headline instantiation is compiled for three waves per SIMD: with the hint hipcc settles on 163-167 VGPRs and a schedule
// worth 1.2 % at 4096 envs, 2.6 % in the 20-step shape; compiled for two it loses 3 %, for four — 128 VGPRs, 42 spilled — 11 %;
// the two-wave kernel is built for four: 2048 workgroups x 2 waves on 1024 SIMDs)
__global__ __launch_bounds__((SPLIT ? 2 : 1) * kWave, (SPLIT ? 4 : HEADLINE ? 3 : 1)) void rollout_fused_kernel(
    Params P_in, const StateView* Sd, const int* ring_filled_in, RolloutView R, int n_steps, const double* ext_action) {
    static_assert(HEADLINE || !SPLIT, "the two-wave kernel exists for the headline geometry only");
    static_assert(SPLIT || ASSIST == 0, "the env wave assists an ORCA wave: two-wave kernel only");
#ifdef CN_WAVE_TRACE
    const unsigned long long wt_entry = __builtin_amdgcn_s_memrealtime();
    unsigned long long wt_fallbacks = 0ull, wt_ends = 0ull;
#endif
    // The 17 state pointers are needed before and after the step loop and when an episode ends — never inside a step — so
    // they stay in the engine's device copy of the StateView and are re-read where used (scalar loads) instead of holding
    // 34 SGPRs (and spilling as many into VGPR lanes) across the loop.  ring_filled_in is the one pointer the host swaps
    // between launches, hence a direct argument.
    constexpr int MAXL = 5;
    Params P = P_in;
    P.async_fill = 0;  // (rollout_route: never beside the asynchronous fill — scenario_ready is the fill-level comparison)
    if (HEADLINE) {  // BASELINE configs[1]: 5 humans + robot, 2 envs per wave, 60 pairs, as compile-time constants
        P.A = 6, P.NC = 5, P.E = 2, P.nA = 12, P.pairs = 60, P.threads = 64;
    }
    const Smem s = carve<MAXL>(P);
    if constexpr (SPLIT) {
        if (__builtin_amdgcn_readfirstlane((int)threadIdx.x) >= kWave) {
            split_orca_wave<MAXL, ASSIST>(P, s, n_steps);
            return;
        }
    }
    const Lane L = lane_of(P);
    AgentRegs r = {};
    float robot_max_speed = 0.0f;
    const bool robot = L.valid && L.a == 0;
    // the ~20 pointers of the io block are needed at launch start / end and when an episode ends: they are re-read from
    // the device copy there (scalar loads) instead of occupying SGPRs across the step loop
    const cn_rollout_io* iop = R.io;
    double theta = 0.0;
    EpisodeBook ep = {};  // (state = kRetired)
    {
        // Launch prologue in TWO memory round trips: every pointer it needs in one batch of scalar loads (both structs are
        // dead again before the step loop), then every per-lane value in one batch of vector loads — unconditional, on clamped
        // indices, so that none waits for another's result (the robot's captured radii are read speculatively: the buffers
        // exist whether or not the policy's simulator has been built).  As a chain of `S->field[..]` / `io->field[..]` reads
        // under their own conditions this was a dozen dependent trips, ~4 of the 113 us of a 20-step launch.
        const StateView S = *Sd;
        const cn_rollout_io io = *iop;
        const size_t gi = L.valid ? L.gi : 0;
        const int env = L.valid ? L.env : 0;
        const double2 p0 = S.pos[gi], v0 = S.vel[gi], g0 = S.goal[gi], q0 = S.rv[gi];
        const bool have = P.robot_orca ? S.rsim_valid[env] != 0 : false;
        const float rr_kept = P.robot_orca ? S.rsim_radius[gi] : 0.0f;
        const float ms_kept = P.robot_orca ? S.rsim_max_speed[env] : 0.0f;
        const double theta0 = S.theta[env];
        EpisodeBook ep0;
        CN_LOAD_EPISODE(P, ep0, S, io, ring_filled_in, env);
        if (L.valid) {
            r.px = p0.x, r.py = p0.y, r.vx = v0.x, r.vy = v0.y, r.gx = g0.x, r.gy = g0.y, r.rad = q0.x, r.vpref = q0.y;
            ep = ep0;  // (every lane of the env: the book is carried redundantly, see the step loop)
            if (L.a == 0) theta = theta0;
            if (P.robot_orca) {  // load_robot_view (step_kernels.h), without its dependent loads
                const float rr = have ? rr_kept : (float)(r.rad + 0.01 + P.robot_safety);
                if (!have) S.rsim_radius[L.gi] = rr;
                s.rview[L.lane] = rr;
                if (L.a == 0) {
                    robot_max_speed = have ? ms_kept : (float)r.vpref;
                    if (!have) S.rsim_max_speed[L.env] = robot_max_speed;
                }
            }
        }
    }
    build_pairs(P, s);

    if (L.valid && ep.state == kWaitingScenario && scenario_ready(P, *Sd, L.env, ep.ep_count, ep.ring_filled)) {  // produced since
        load_from_ring(P, *Sd, L, ep.ep_count % P.ring_mod, r);
        ep.state = kRunning;
        ep.gtime = 0.0;
        theta = 1.5707963267948966;
    }
    unsigned int transitions = 0;
    for (int t = threadIdx.x; t < kMaxDiscount; t += P.threads) s.disc[t] = t < R.discount_len ? R.discount[t] : 0.0;
    CN_FUSED_SYNC();  // pinfo, rview
    if (L.lane == 0) s.kin[P.nA] = make_float4(std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity(), 0.0f, 0.0f);
    const PairRow pr = pair_row_of(P, s, L.lane);
    const StepConsts K = step_consts(P);
    // two-wave kernel: the ORCA wave owns kin (it stages the next view itself, ahead of barrier 1); the env wave's true rows of
    // a (re)started episode go to d2, free in the fused kernels (headline geometry: 60 floats for 12 rows of 16 bytes, 16-byte aligned)
    float4* const kin_stage = SPLIT ? reinterpret_cast<float4*>(s.d2) : s.kin;
    stage_agent(P, s, L, r, K.hsafety, kin_stage);
    CN_FUSED_SYNC();

#ifdef CN_PHASE_TIMING
    PhaseClock clock = {};
    PhaseClock* clk = &clock;
    clock.last = __builtin_readcyclecounter();
#else
    PhaseClock* clk = nullptr;
    (void)clk;
#endif
    const float range_sq = P.orca.neighbor_dist * P.orca.neighbor_dist;
#ifdef CN_WAVE_TRACE
    const unsigned long long wt_loop = __builtin_amdgcn_s_memrealtime();
#endif
    if constexpr (SPLIT) {
        float2* const vel = reinterpret_cast<float2*>(s.act);
        // "re-read the staged state"; no agent predicted infeasible; [2], [3]: episode starts adopted, iterations redone
        if (L.lane == 0) s.flag[0] = 1, s.flag[1] = 0, s.flag[2] = 0, s.flag[3] = 0;
        split_barrier();  // prologue staged
        bool skip = true;  // the state of step u is already in registers: nothing to integrate, nothing to book
        // Mirror lanes: lane 16 + l carries a copy of agent lane l's position and goal (in the same registers: nothing else
        // reads r beyond the agent lanes) and of "its env runs", so that the two divisions of the preferred velocity are ONE
        // sequence on two lane groups.  Copied here and after an episode end (the only places where goal, position or the
        // env's state change other than by Agent.step), integrated by the mirror lanes themselves in between.
        // (headline geometry: 12 agent lanes, so lanes 16-27 are free)
        const bool mirror = L.lane >= 16 && L.lane < 16 + P.nA;
        const int m_lane = L.lane & 15;
        const int m_ebase = __shfl(L.ebase, m_lane);
        const bool m_robot = __shfl((int)(L.a == 0), m_lane) != 0;
        bool m_running = false;
        const auto copy_to_mirror = [&] {
            const double px = __shfl(r.px, m_lane), py = __shfl(r.py, m_lane), gx = __shfl(r.gx, m_lane), gy = __shfl(r.gy, m_lane);
            const int run = __shfl((int)(L.valid && ep.state == kRunning), m_lane);
            if (mirror) r.px = px, r.py = py, r.gx = gx, r.gy = gy, m_running = run != 0;
        };
        copy_to_mirror();
        // Fresh start: an episode that starts from a ring slot whose first step was solved when the slot was filled
        // (ring_first_step_kernel, StateView::ring_vel0) costs the workgroup no redone iteration.  The env wave leaves those
        // velocities in a row of its own — the upper half of Smem::act, behind the ORCA wave's vel — and the lanes of such an
        // env (and their mirror lanes) integrate the episode's first step from that row: v0_off is the row's offset for them in
        // that one iteration, 0 otherwise.  vel holds the dead episode's solve then; the other env reads it as ever.
        int v0_off = 0;
        SPLIT_PROBE_DECL();
        for (int u = 0;;) {
            SPLIT_PROBE_WAIT(0, split_barrier());  // 1: vel(u - 1)
            if (!skip) ++u;
            const unsigned int pred = ((ASSIST & kAssistHead) || kSplitProbe) ? (unsigned int)__builtin_amdgcn_readfirstlane(s.flag[1]) : 0u;
            SPLIT_PROBE_AFTER_1(pred, (ASSIST & kAssistHead) != 0 && split_has_head<MAXL>(pred, u, n_steps));
            const bool running = L.valid && ep.state == kRunning;
            const AgentRegs r0 = r;  // the agent at the start of step u - 1
            double act_x = 0.0, act_y = 0.0, new_vx = 0.0, new_vy = 0.0;
            // (the mirror lanes integrate their copy with the same statements on the same operands: no instruction more)
            if (!skip && (L.lane < P.nA || mirror)) {
                const float2 mine = vel[v0_off + m_lane], robots = vel[v0_off + m_ebase];
                v0_off = 0;
                act_x = (double)robots.x, act_y = (double)robots.y;
                new_vx = m_robot ? act_x : (double)mine.x;
                new_vy = m_robot ? act_y : (double)mine.y;
                if (mirror ? m_running : running) {  // Agent.step (agent.py:127-135)
                    r.px = r.px + new_vx * K.dt;
                    r.py = r.py + new_vy * K.dt;
                    r.vx = new_vx;
                    r.vy = new_vy;
                }
            }
            if (u < n_steps && (L.lane < P.nA || mirror)) {
                // preferred_velocity with ONE float64 division sequence: the agent's lane divides gdx, its mirror lane gdy
                const double gdx = r.gx - r.px, gdy = r.gy - r.py;
                const double speed = norm2(gdx, gdy);
                const double num = mirror ? gdy : gdx;
                const float pref = (float)(speed > 1.0 ? num / speed : num);
                // rows of 16 lanes: row 1 of the first operand <-> row 0 of the second, so [1] holds the mirror lanes' value on
                // the agent lanes
                const float pref_y = __uint_as_float(__builtin_amdgcn_permlane16_swap(__float_as_uint(pref), __float_as_uint(pref), false, false)[1]);
                if (L.lane < P.nA) {
                    const float max_speed = (L.a == 0) ? robot_max_speed : (float)r.vpref;
                    float sx, sy;
                    lp_start_point(max_speed, pref, pref_y, sx, sy);
                    s.sol[L.lane] = make_float4(pref, pref_y, max_speed, (running && (L.a > 0 || P.robot_orca)) ? 1.0f : 0.0f);
                    s.res[L.lane] = make_float4(sx, sy, 0.0f, 0.0f);
                }
            }
            SPLIT_PROBE_WAIT(1, split_barrier());  // 2
            if constexpr ((ASSIST & kAssistHead) != 0) {
                if (split_has_head<MAXL>(pred, u, n_steps)) {  // lines and sol of step u are complete: the fallback's head
                    __builtin_amdgcn_s_setprio(CN_SPLIT_HEAD_PRIO);
                    const Lp3Item it = lp3_item_of<MAXL>(s, L.lane, (unsigned long long)pred);
                    lp3_head<MAXL>(s, it);
                    __builtin_amdgcn_s_setprio(CN_SPLIT_HEAD_TAIL_PRIO);
                    SPLIT_PROBE_WAIT(2, split_barrier());  // 3
                }
            }
            bool ended = false;
            unsigned int adopt = 0u;
            bool done = false, v0_ok = false;  // v0_ok: the env went on with a scenario whose first step is solved (v0)
            float2 v0 = make_float2(0.0f, 0.0f);
            if (!skip) {
                // the robot's position at the start of the step: from its lane's registers (posd holds re-staged states only)
                const double2 rp = make_double2(__shfl(r0.px, L.ebase), __shfl(r0.py, L.ebase));
                if (L.valid) s.closest[L.lane] = swept_distance(r0, L.a > 0, rp, act_x, act_y, new_vx, new_vy, K.dt, s.rad[L.ebase]);
                CN_FUSED_SYNC();
                if (running) {
                    const double disc_t = s.disc[ep.cur_steps < kMaxDiscount ? ep.cur_steps : kMaxDiscount - 1];
                    const StepOutcome o = reduce_env(P, s, L.ebase, ep.gtime, K);
                    done = o.done;
                    ep.gtime += K.dt;
                    ++transitions;
                    CN_BOOK_TRANSITION(ep, ep.cur_steps < kMaxDiscount ? disc_t : 0.0, o.reward, o.info, o.dmin);
                    if (done) {  // explorer.py:50-72: record, then the env's next episode
                        // every load of the episode end first (the io block, the state pointers, the next scenario and its solved
                        // first step — in bounds whether or not it is taken; an engine that runs this kernel has the ring_vel0
                        // arrays: ScenarioRing::first_step), then the record stores: one memory round trip in the shadow of the
                        // ORCA wave's step
                        const cn_rollout_io io = *iop;
                        const StateView S = *Sd;
                        AgentRegs next = r;
                        const int next_slot = (ep.ep_count + 1) % P.ring_mod;
                        load_from_ring(P, S, L, next_slot, next);
                        const size_t next_idx = (size_t)L.env * P.ring_mod + next_slot;
                        const float2 v0_next = S.ring_vel0[next_idx * P.A + L.a];
                        const bool ok_next = S.ring_vel0_ok[next_idx] != 0;
                        CN_END_EPISODE(P, S, io, L.env, L.a == 0, K.limit, o.info, ep,
                                       r = next; theta = 1.5707963267948966; v0 = v0_next; v0_ok = ok_next);
                    }
                }
                const unsigned long long ended_lanes = __ballot(done);
                ended = ended_lanes != 0ull;
                // fresh (wave-uniform): every env that ended goes on, from a solved first step, and the launch has a step left for
                // it.  Then nothing is redone: bit 1 + el of the word tells the ORCA wave that env el adopts what is staged below
                if (ended && u < n_steps && __ballot(done && v0_ok) == ended_lanes)
                    for (int el = 0; el < P.E; ++el) adopt |= (unsigned int)((ended_lanes >> (el * P.A)) & 1ull) << (1 + el);
            }
            // per-episode constants (rad, hview) and the float32 view are staged here and in the prologue only.  Not fresh: the
            // true state of step u.  Fresh: the restarted envs' lanes stage the state BEHIND the solved step — the ORCA wave's own
            // staging expression; the integration of the next iteration yields the same bits — and keep the velocities for it;
            // what the other env's lanes stage nobody reads.
            if (ended) {
                AgentRegs st = r;
                if (adopt != 0u && done) {
                    st.px = r.px + (double)v0.x * K.dt;
                    st.py = r.py + (double)v0.y * K.dt;
                    st.vx = (double)v0.x, st.vy = (double)v0.y;
                    vel[P.nA + L.lane] = v0;
                }
                stage_agent(P, s, L, st, K.hsafety, kin_stage);
                copy_to_mirror();
                if (adopt != 0u) v0_off = ((adopt >> (1 + m_ebase / P.A)) & 1u) != 0u ? P.nA : 0;
                // counted in two LDS words of the env wave's own and added to StateView::fresh_counts behind the loop: a global
                // atomic here — the pointer's load, then the atomic — was a dependent memory round trip in front of barrier 1
                // (the last step of a launch: its end costs no iteration either way)
                if (L.lane == 0 && u < n_steps) s.flag[adopt != 0u ? 2 : 3] += adopt != 0u ? __popc(adopt) : 1;
            }
            if (L.lane == 0) s.flag[0] = ended ? (adopt != 0u ? (int)adopt : 1) : 0;
            skip = ended && adopt == 0u;
            if constexpr ((ASSIST & kAssistHead) != 0 && CN_SPLIT_HEAD_TAIL_PRIO != 0) __builtin_amdgcn_s_setprio(0);
            if (u >= n_steps) break;
        }
        SPLIT_PROBE_FLUSH(L.lane, 10);
    }
    const int one_wave_steps = SPLIT ? 0 : n_steps;
    for (int step = 0; step < one_wave_steps; ++step) {
        const bool running = L.valid && ep.state == kRunning;
        const bool solve = running && (L.a > 0 || P.robot_orca);

        // ---- pairs: candidate distances (Appendix A.2), stable rank = RVO2's sorted-insertion slot, half-plane (A.3)
        if (L.lane < P.pairs) {
            // (agent lanes are pair lanes too: their preferred velocity, same block)
            float4 sol4, start4;
            fused_pair_phase(P, s, pr, range_sq, pair_rsum(s, pr), [&] {
                preferred_velocity(r, (L.a == 0) ? robot_max_speed : (float)r.vpref, solve, sol4, start4);
            });
            if (L.lane < P.nA) {
                s.sol[L.lane] = sol4;
                s.res[L.lane] = start4;
            }
        }
        CN_FUSED_SYNC();
        CN_TICK(clk, 2);

        // ---- candidates: lane = (agent, half-plane)
        fused_candidates<MAXL>(P, s, L.lane);
        CN_FUSED_SYNC();

        // ---- solve: scan, then the candidate-form fallback for the infeasible agents
        float rx, ry;
        const bool fell_back = fused_solve<MAXL>(P, s, L.lane, solve, rx, ry, clk) != 0ull;
        (void)fell_back;
#ifdef CN_WAVE_TRACE
        if (fell_back) ++wt_fallbacks;
#endif
        CN_TICK(clk, 8);

        // ---- the robot's action reaches every lane of its env (wave shuffle; caller-supplied actions: one load per lane)
        double act_x, act_y;
        if (P.robot_orca) {
            act_x = (double)__shfl(rx, L.ebase);
            act_y = (double)__shfl(ry, L.ebase);
        } else {
            act_x = L.valid ? ext_action[2 * (size_t)L.env] : 0.0;
            act_y = L.valid ? ext_action[2 * (size_t)L.env + 1] : 0.0;
        }
        const double new_vx = (L.a == 0) ? act_x : (double)rx;
        const double new_vy = (L.a == 0) ? act_y : (double)ry;

        // ---- one float64 distance per agent lane (crowd_sim.py:331-351 for a human, :364-366 for the robot)
        if (L.valid)
            s.closest[L.lane] = swept_distance(r, L.a > 0, s.posd[L.ebase], act_x, act_y, new_vx, new_vy, K.dt, s.rad[L.ebase]);
        CN_FUSED_SYNC();
        CN_TICK(clk, 5);

        // ---- reduce (every lane of the env, identically), integrate, episode bookkeeping, stage the next step
        if (running) {
            const double disc_t = s.disc[ep.cur_steps < kMaxDiscount ? ep.cur_steps : kMaxDiscount - 1];
            const StepOutcome o = reduce_env(P, s, L.ebase, ep.gtime, K);
            const double reward = o.reward, dmin = o.dmin;
            const int info = o.info;
            const bool done = o.done;
            ep.gtime += K.dt;
            r.px = r.px + new_vx * K.dt;  // Agent.step (agent.py:127-135)
            r.py = r.py + new_vy * K.dt;
            r.vx = new_vx;
            r.vy = new_vy;
            // the book: every lane of the env carries it (only the robot lane's copy is written out)
            ++transitions;
            CN_BOOK_TRANSITION(ep, ep.cur_steps < kMaxDiscount ? disc_t : 0.0, reward, info, dmin);
#ifdef CN_WAVE_TRACE
            if (__ballot(done) != 0ull) ++wt_ends;
#endif
            if (done) {  // explorer.py:50-72: record, then the env's next episode
                const cn_rollout_io io = *iop;
                CN_END_EPISODE(P, *Sd, io, L.env, L.a == 0, K.limit, info, ep,
                               load_from_ring(P, *Sd, L, ep.ep_count % P.ring_mod, r); theta = 1.5707963267948966);
            }
        }
        stage_agent(P, s, L, r, K.hsafety, kin_stage);
        CN_FUSED_SYNC();
        CN_TICK(clk, 7);
    }
#ifdef CN_PHASE_TIMING
    if ((threadIdx.x & (kWave - 1)) == 0) {
        unsigned long long total = 0ull;
        for (int k = 0; k < 10; ++k) {
            atomicAdd(&cn_phase_cycles[k], clock.acc[k]);
            if (k != 9) total += clock.acc[k];
        }
        atomicMax(&cn_phase_cycles[14], total);  // the slowest wave's step loop (what a launch waits for) ...
        atomicMin(&cn_phase_cycles[13], total);  // ... and the fastest one's (reset to ~0ull by the probe script)
        atomicAdd(&cn_phase_cycles[15], 1ull);
    }
#endif

#ifdef CN_WAVE_TRACE
    const unsigned long long wt_exit = __builtin_amdgcn_s_memrealtime();
#endif
    const StateView S = *Sd;
    if constexpr (SPLIT) {
        if (L.lane == 0) {
            const int adopted = s.flag[2], redone = s.flag[3];
            if (adopted != 0) atomicAdd(&S.fresh_counts[0], (unsigned int)adopted);
            if (redone != 0) atomicAdd(&S.fresh_counts[1], (unsigned int)redone);
        }
    }
    if (L.valid) CN_STORE_AGENT(S, L.gi, r);
    const cn_rollout_io io = *iop;
    if (robot) CN_STORE_EPISODE(P, S, io, L.env, ep, theta);
    // transitions counter, record blocks, explorer.py:74-90 sums: the launch's own tail (rollout_kernels.h: rollout_epilogue)
    rollout_epilogue(P, S, io, L, robot, transitions, ep.ep_count, reinterpret_cast<double*>(s.lines));
#ifdef CN_WAVE_TRACE
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
        unsigned long long* w = cn_wave_trace + 6 * blockIdx.x;
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        w[0] = wt_entry, w[1] = wt_loop, w[2] = wt_exit, w[3] = __builtin_amdgcn_s_memrealtime();
        w[4] = wt_fallbacks | (wt_ends << 32), w[5] = hw;
    }
#endif
}

// ---------------------------------------------------------------------------------------------- first steps, at fill time
// The first ORCA step of a ring scenario is a pure function of the scenario (velocities zero), the engine's parameters and the
// robot's captured simulator: solved HERE, once, behind the fill that generated the scenario (ScenarioRing::around_launch, on the
// fill's stream), so that the two-wave kernel above starts the episode without redoing that step.  The one-wave headline layout
// — one wave per workgroup, two jobs (ring slots of StateView::first_list) per wave, 12 agent lanes, 60 pair lanes — and the
// one-wave kernel's own phase bodies, once each; no swept distance, no integration, no bookkeeping.  A fixed grid strides over the
// list (a plain bounded loop, as ring_redo_kernel's).  The robot's view follows load_robot_view's rule on the data the next
// launch's prologue will find: captured radii and top speed where rsim_valid says so, else what that prologue will capture from
// the env's current state.  The host enqueues the kernel only where that data cannot change under it.
constexpr int kFirstStepWgs = 2048;
__global__ __launch_bounds__(kWave) void ring_first_step_kernel(Params P_in, StateView S) {
    constexpr int MAXL = 5;
    Params P = P_in;
    P.A = 6, P.NC = 5, P.E = 2, P.nA = 12, P.pairs = 60, P.threads = 64;
    const Smem s = carve<MAXL>(P);
    const int lane = threadIdx.x;
    const int el = lane / P.A;
    const bool agent = lane < P.nA;
    build_pairs(P, s, true);
    if (lane == 0) s.kin[P.nA] = make_float4(std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity(), 0.0f, 0.0f);
    CN_FUSED_SYNC();
    const PairRow pr = pair_row_of(P, s, lane);
    const float range_sq = P.orca.neighbor_dist * P.orca.neighbor_dist;
    const int slots = P.B * P.ring_mod;
    const int listed = __builtin_amdgcn_readfirstlane(S.redo_count[1]);
    const int n = listed < slots ? listed : slots;
    for (int k = 2 * (int)blockIdx.x; k < n; k += 2 * kFirstStepWgs) {
        // the wave's second env is job k + 1, or job k once more where the list ends (computed, not stored)
        const bool both = k + 1 < n;
        const int listed_idx = S.first_list[k + ((el == 1 && both) ? 1 : 0)];
        const int ring_idx = listed_idx < 0 ? 0 : (listed_idx < slots ? listed_idx : slots - 1);
        Lane L;
        L.lane = lane, L.a = lane - el * P.A, L.ebase = el * P.A, L.env = ring_idx / P.ring_mod, L.valid = agent;
        L.gi = (size_t)L.env * P.A + (agent ? L.a : 0);
        const size_t ri = (size_t)ring_idx * P.A + (agent ? L.a : 0);
        // every load of the job in one batch, unconditional on in-bounds indices
        const double2 p = S.ring_pos[ri], g = S.ring_goal[ri], q = S.ring_rv[ri], cur = S.rv[L.gi];
        const bool have = S.rsim_valid[L.env] != 0;
        const float rr_kept = S.rsim_radius[L.gi], ms_kept = S.rsim_max_speed[L.env];
        AgentRegs r;  // (load_from_ring's)
        r.px = p.x, r.py = p.y, r.vx = 0.0, r.vy = 0.0, r.gx = g.x, r.gy = g.y, r.rad = q.x, r.vpref = q.y;
        const float robot_max_speed = have ? ms_kept : (float)cur.y;
        if (agent) s.rview[lane] = have ? rr_kept : (float)(cur.x + 0.01 + P.robot_safety);
        stage_agent(P, s, L, r, P.human_safety, s.kin);
        CN_FUSED_SYNC();
        if (lane < P.pairs) {
            float4 sol4, start4;
            fused_pair_phase(P, s, pr, range_sq, pair_rsum(s, pr), [&] {
                preferred_velocity(r, (L.a == 0) ? robot_max_speed : (float)r.vpref, agent, sol4, start4);
            });
            if (agent) {
                s.sol[lane] = sol4;
                s.res[lane] = start4;
            }
        }
        CN_FUSED_SYNC();
        fused_candidates<MAXL>(P, s, lane);
        CN_FUSED_SYNC();
        float rx, ry;
        fused_solve<MAXL>(P, s, lane, agent, rx, ry, nullptr);
        if (agent && (el == 0 || both)) {
            S.ring_vel0[ri] = make_float2(rx, ry);
            if (L.a == 0) S.ring_vel0_ok[ring_idx] = 1;
        }
        CN_FUSED_SYNC();
    }
}

}  // namespace cn
