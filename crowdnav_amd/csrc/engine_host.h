// Host side shared by the translation units of libcrowdnav_amd.so: the engine object behind the opaque cn_engine handle, error
// text, the slab allocator and the launch helpers.  Every *.hip of this directory is one unit and one code object, compiled side
// by side, no device symbol shared between them: crowdnav_amd.hip holds the env / rollout entry points and their kernels,
// sarl_abi.hip the value-network decision (cn_sarl_*) and the kernels around the network, sarl_lds.hip / sarl_reg.hip /
// sarl_reg_chunk.hip / sarl_reg_seq.hip / sarl_f16.hip the network's kernel families behind sarl_host.h, sarl_train.hip the SGD step, plan.hip the
// planners and predictors.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/crowdnav_amd.h"
#include "fill_plan.h"
#include "step_kernels.h"


// ------------------------------------------------------------------------------------------------ C ABI

// thread-local text of the last failure (cn_last_error); one definition, in crowdnav_amd.hip
extern thread_local char cn_g_err[512];

namespace {

[[maybe_unused]] int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(cn_g_err, sizeof(cn_g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define CN_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t err__ = (call);                                                                \
        if (err__ != hipSuccess)                                                                  \
            return fail(CN_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, \
                        __LINE__);                                                                \
    } while (0)

}  // namespace

// Host side of the scenario ring: what cn_rollout_begin and the cn_rollout_* entry points keep about the ring between calls.
// The methods are scenario_ring_host.h's (crowdnav_amd.hip only); the device side is scenario_ring.h, the rule for when a fill
// runs fill_plan.h.  The ring's device buffers are StateView's ring_* / redo_* / cache_* pointers, allocated by create().
struct ScenarioRing {
    // Where a fill runs.  InFront: on the engine's stream, in front of the launch that needs it.  Beside: the lagged fill of the
    // lane-per-scenario generators, on fill_streams[0] beside a launch, one call ahead (the ring then has 2 D slots per env).
    // WorkList: CN_FLAG_ASYNC_SCENARIO_FILL with the wave-per-scenario generators — a scan + job-list launch per transition
    // launch, round-robin over the side streams (a launch stuck on a hard scenario must not hold back the next one), each
    // starting once the previous transition kernel has written its episode counters; slots are published one by one.
    enum class Fill { InFront, Beside, WorkList };
    static constexpr int kFillStreams = 8;
    bool gen_wave = false;       // wave-per-scenario generators (64 rejection attempts at a time): long chains, H > 8
    Fill mode = Fill::InFront;
    bool scenario_cache = true;  // wave generators keep the scenarios of a small seed set (CROWDNAV_AMD_SCENARIO_CACHE)
    cn::FillPlan plan;           // InFront / Beside: which calls fill, and when the two level buffers change hands
    hipStream_t fill_streams[kFillStreams] = {};
    hipEvent_t rollout_done = nullptr;  // on the engine's stream: everything in front of the launch a fill runs beside
    hipEvent_t fill_done = nullptr;     // Beside: the fill's end, which the launch that takes its levels waits for
    int next_fill_stream = 0;
    int* fill_list = nullptr;    // [kFillStreams][2 + 2 B D] job lists of ring_fill_scan_kernel / ring_fill_jobs_kernel, one per side stream
    int fill_queue_wgs = 1;      // persistent generator workgroups of a WorkList fill launch (CROWDNAV_AMD_FILL_QUEUE_WGS, at least 1)
    int* ep_snap = nullptr;      // [B] the Beside fill's copy of StateView::ep_word (ring_fill_begin_kernel)
    uint64_t lagged_fills = 0;   // cn_lagged_fills: fills enqueued beside a launch (counted in CN_COUNT_RING_FILLS too)
    // First step of every scenario solved at fill time (rollout_fused.h: ring_first_step_kernel).
    bool first_step = false;     // the engine's cn_rollout runs the two-wave kernel (read_knobs): its fills clear ring_vel0_ok, list
                                 // their slots and are followed by the kernel
    bool robot_sim_known = false;  // every env's rsim_* is captured and complete in stream order behind whatever the engine's stream
                                   // holds now: a rollout launch was enqueued, or cn_set_robot_sim, and no drop since.  Only then may
                                   // the kernel run BESIDE a launch — that launch's prologue might otherwise be the one that captures
    uint64_t first_step_kernels = 0;  // ring_first_step_kernel launches enqueued (cn_fresh_starts)

    void configure(cn_engine* e, int compute_units);
    int create(cn_engine* e);
    void destroy();
    int begin(cn_engine* e, uint32_t seed_mod);
    template <class Launch>
    int around_launch(cn_engine* e, int n_steps, Launch&& launch);
    int settle(cn_engine* e);
    int drain(cn_engine* e);
    int forget_first_steps(cn_engine* e);
};

struct cn_engine {
    cn_config cfg{};
    cn::Params P{};
    cn::ScenarioCfg C{};
    cn::StateView S{};
    hipStream_t stream = nullptr;
    cn_rollout_io io_host{};           // last cn_rollout_io uploaded to io_dev
    cn_rollout_io* io_dev = nullptr;   // device copy the rollout kernels read through
    cn::StateView* S_dev = nullptr;    // device copy of S (the fused rollout kernel re-reads state pointers instead of holding them)
    cn_lookahead_out look_host{};          // last cn_lookahead_out uploaded to look_dev (look_valid: there is one)
    cn_lookahead_out* look_dev = nullptr;  // device copy rollout_lookahead_kernel stores through; room for two: the double at
                                           // look_dev + 1 is the weight rollout_lookahead_goal_kernel reads (look_goal_dev)
    bool look_valid = false;
    int look_human_model = CN_HUMANS_ORCA;  // cn_lookahead_set_human_model: read by cn_lookahead_actions and by nothing else
    double look_goal_weight = 0.0;  // cn_lookahead_set_goal_weight: != 0 launches the goal forms of the four lookahead kernels
    double look_goal_dev = 0.0;     // the weight last uploaded behind look_dev (the slab is zeroed: 0.0 until one is)
    double plan_max_rotation = 0.0;  // cn_plan_set_unicycle: R > 0 opts a CN_UNICYCLE engine into the cn_plan_* calls, rows (v, r)
    double plan_std_rotation = 0.0;  // ... and the initial deviation of r (cfg->init_std stays v's)
    ScenarioRing ring;
    bool io_valid = false;
    bool rollout_begun = false;          // cn_rollout_begin has run: the seed numbering below is fixed until the next one
    uint32_t begin_seed_base = 0, begin_seed_mod = 0;  // (the scenario cache is sized and keyed by them)
    struct cn_sarl* sarl = nullptr;  // SARL decision state (sarl_abi.hip), NULL until cn_sarl_configure
    bool orca_fresh = false;  // cn_sarl_sample_step: the humans' ORCA velocities of the CURRENT state are in sarl->orca_vel (left by the
                              // previous call's transition kernel); cleared by every other entry point (bind)
    double* discount = nullptr;
    int discount_len = 0;
    uint32_t* probe_key = nullptr;
    double* summary_scratch = nullptr;  // records_summary_kernel: per-workgroup partials + ticket counter
    int maxl = 10;           // half-planes held in VGPRs by the solve phase: 5 or 10
    size_t smem = 0;         // dynamic LDS bytes per workgroup
    int sched_min = 0, sched_slots = 0, sched_reserve = 0, dyn_visits = 0;  // the 20-human shard kernel's schedules (launch_shard): shortest call split, resident workgroups, slots left free beside the asynchronous fill
    bool sched_force = false, sched_dynamic = true;
    bool use_fused = true;  // CROWDNAV_AMD_FUSED (rollout_route)
    int fused_split = 1;    // CROWDNAV_AMD_FUSED_SPLIT: 0 never, 1 launches of one round (default), 2 always
    int split_assist = 0;   // CROWDNAV_AMD_SPLIT_ASSIST: rollout_fused.h's ASSIST (0, or kAssistHead = fallback head on the env wave; default)
    int split_slots = 0;    // workgroups of the two-wave fused kernel the device holds at once (occupancy query, read_knobs)
    uint64_t launch_counts[CN_LAUNCH_COUNTERS] = {};  // cn_launch_counts: what the host enqueued since cn_create
    // Device memory comes from a few large slabs, not one hipMalloc per buffer: an engine has ~60 device buffers, most of them a
    // few KiB; one 32 MiB slab (plus one per buffer larger than that) is 2-4 mappings to create and - each hipFree being a device
    // synchronisation - 2-4 to tear down, and cn_sarl_configure can roll a failed configuration back to a mark.
    struct Slab {
        char* base;
        size_t size, used;
    };
    std::vector<Slab> slabs;
    struct AllocMark {  // fill level of every slab that existed at the mark
        std::vector<size_t> used;
    };
    AllocMark alloc_mark() const {
        AllocMark m;
        for (const Slab& s : slabs) m.used.push_back(s.used);
        return m;
    }
    void alloc_rollback(const AllocMark& m) {  // frees everything allocated since alloc_mark()
        while (slabs.size() > m.used.size()) {
            (void)hipFree(slabs.back().base);
            slabs.pop_back();
        }
        for (size_t i = 0; i < slabs.size(); ++i) slabs[i].used = m.used[i];
    }
};

namespace {

constexpr size_t kSlabBytes = (size_t)32 << 20, kSlabAlign = 4096;

template <typename T>
int dev_alloc(cn_engine* e, T** out, size_t n) {
    const size_t bytes = (n * sizeof(T) + kSlabAlign - 1) / kSlabAlign * kSlabAlign;
    // first fit over ALL slabs: a buffer larger than a slab gets one of its own, exactly sized (so it is full and never
    // chosen again), and the small buffers that follow keep filling the shared slab they were filling before — looking at
    // the newest slab only stranded up to 32 MiB at every large / small alternation of cn_sarl_configure
    size_t k = 0;
    while (k < e->slabs.size() && e->slabs[k].used + bytes > e->slabs[k].size) ++k;
    if (k == e->slabs.size()) {
        const size_t size = bytes > kSlabBytes ? (bytes + ((size_t)2 << 20) - 1) >> 21 << 21 : kSlabBytes;
        void* p = nullptr;
        CN_HIP(hipMalloc(&p, size));
        e->slabs.push_back({static_cast<char*>(p), size, 0});
    }
    cn_engine::Slab& sl = e->slabs[k];
    void* p = sl.base + sl.used;
    sl.used += bytes;
    CN_HIP(hipMemset(p, 0, bytes));
    *out = static_cast<T*>(p);
    return CN_OK;
}

[[maybe_unused]] int bind(cn_engine* e) {
    if (!e) return fail(CN_ERR_INVALID, "engine is NULL");
    e->orca_fresh = false;  // whatever this call is, it may change the state those velocities belong to
    CN_HIP(hipSetDevice(e->cfg.device));
    return CN_OK;
}

inline int grid_envs(const cn_engine* e) { return (e->P.B + e->P.E - 1) / e->P.E; }

// Run-time values as template arguments: f(std::integral_constant<int, V>{}) for the V of the list that equals v (false: none
// does), f(std::true_type{}) or f(std::false_type{}).  A launch names its kernel as kernel<decltype(v)::value, ...>; every
// combination of the listed values is instantiated.
template <int... Vs, class F>
inline bool pick_int(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <class F>
inline void pick_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// ... the engine's half-plane capacity: 5, or 10 for everything else
template <class F>
inline void pick_maxl(const cn_engine* e, F&& f) {
    if (!pick_int<5>(e->maxl, f)) f(std::integral_constant<int, 10>{});
}
// ... with the robot kinematics (the unicycle code only exists in the UNI instantiations) and the kd-tree bookkeeping of
// simulators with more than 10 agents: step_kernel<MAXL, UNI, KD>, rollout_kernel<MAXL, UNI, HEADLINE, KD>
template <class F>
inline void pick_maxl_uni_kd(const cn_engine* e, F&& f) {
    pick_maxl(e, [&](auto maxl) {
        pick_bool(e->P.robot_unicycle, [&](auto uni) { pick_bool(e->P.kd, [&](auto kd) { f(maxl, uni, kd); }); });
    });
}

// Goal form or plain form of a lookahead kernel (cn_lookahead_set_goal_weight): the one place that decides it, for the four
// lookahead launch sites.  A weight of exactly 0.0 (-0.0 included) launches the kernels that know nothing of the term.
inline bool look_goal(const cn_engine* e) { return e->look_goal_weight != 0.0; }
// ... beside the robot kinematics: f(uni, goal)
template <class F>
inline void pick_uni_goal(const cn_engine* e, F&& f) {
    pick_bool(e->P.robot_unicycle, [&](auto uni) { pick_bool(look_goal(e), [&](auto goal) { f(uni, goal); }); });
}

[[maybe_unused]] int env_int(const char* name, int fallback) {
    const char* v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : fallback;
}
inline int grid_lanes(const cn_engine* e) { return (e->P.B + cn::kWave - 1) / cn::kWave; }

}  // namespace


// sarl_abi.hip: frees the host part of the SARL state (device buffers are the engine's slabs)
void cn_sarl_release(cn_engine* e);
// crowdnav_amd.hip: launches orca_kernel (the kernels of step_kernels.h are instantiated in that translation unit only; plan.hip
// builds its own predict_orca_kernel from the same device functions)
void cn_launch_orca(cn_engine* e, float* out_vel);
// crowdnav_amd.hip: cn_lookahead_actions' refusals, in its order and with its messages; CN_OK: the call would launch (or, with
// n_steps == 0, do nothing)
int cn_lookahead_check(const cn_engine* e, int n_steps, int n_candidates, const double* actions, const cn_lookahead_out* out);
