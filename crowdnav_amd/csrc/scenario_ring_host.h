// Host side of the scenario ring (the methods of engine_host.h's ScenarioRing), for crowdnav_amd.hip alone: the kernels it
// launches are scenario_ring.h's.  Its callers know five things.  configure / create / destroy: the generator family, where a
// fill runs (ScenarioRing::Fill), the ring's size, its device buffers, streams and events.  begin: cn_rollout_begin's restart.
// around_launch: the one way a transition kernel is launched on a ring.  settle and drain: the two ways to wait for fills that
// are still out.  WHEN a fill runs, and when the two level buffers change hands, is fill_plan.h's rule; this file executes it.
#pragma once
#include "engine_host.h"
#include "rollout_fused.h"  // (ring_first_step_kernel runs the fused kernels' phase bodies; scenario_ring.h comes with it)

// The launch reads StateView::ring_filled_in; a fill reads it too and writes ring_filled_out.  Once per fill the two change
// hands: at once for a fill in front of the launch, when FillPlan says so (Decision::take_levels, settle()) for one beside it.
static inline void swap_levels(cn::StateView& S) { std::swap(S.ring_filled_in, S.ring_filled_out); }

// The generator family, where the fills run, and the ring's size that follows from both.  compute_units: the device's.
inline void ScenarioRing::configure(cn_engine* e, int compute_units) {
    const cn_config* c = &e->cfg;
    cn::Params& P = e->P;
    gen_wave = env_int("CROWDNAV_AMD_WAVE_SCENARIOS", c->num_humans > 8 ? 1 : 0) != 0;
    // Lagged fill (fill_plan.h; CROWDNAV_AMD_LAGGED_FILL, default on): the lane-per-scenario generator's ring gets 2 D slots per
    // env and its top-ups run on a side stream beside the launches.  0: D slots, every fill in front of the launch that needs it.
    // It pays where a launch is ONE round of workgroups: its waves then run in the launch's tail.  Beside a launch of several
    // rounds they take slots from queued workgroups instead (32768 envs: 1.2 % slower than the fill in front).  Two waves per
    // SIMD is what every rollout kernel fits: 8 one-wave workgroups per CU.
    if ((c->flags & CN_FLAG_ASYNC_SCENARIO_FILL) != 0 && gen_wave) mode = Fill::WorkList;
    else if (!gen_wave && env_int("CROWDNAV_AMD_LAGGED_FILL", 1) != 0 && grid_envs(e) <= 8 * compute_units) mode = Fill::Beside;
    else mode = Fill::InFront;
    P.async_fill = mode == Fill::WorkList ? 1 : 0;
    // Asynchronous fill: a slot is refilled by the fill launch AFTER the call that consumed it, behind up to one call's worth of
    // other scenarios, and a hard scenario of the reference geometry (20 humans on the 4 m circle: up to 3 M attempts) is tens
    // of milliseconds of one wave — so the ring is the latency buffer.  Measured (r06, 4096 x 20, 999-step calls, every
    // scenario generated afresh): depth 48 / 96 / 144 = 16 % / 3 % / 0 % of the env-steps paused.  0.6 GB of the 288.
    P.ring_depth = env_int("CROWDNAV_AMD_RING_DEPTH", 48);
    if (P.ring_depth < 1) P.ring_depth = 1;
    if (mode == Fill::WorkList && !getenv("CROWDNAV_AMD_RING_DEPTH")) P.ring_depth = 144;
    plan.configure(P.ring_depth, mode == Fill::Beside);
    P.ring_mod = plan.C;
    scenario_cache = env_int("CROWDNAV_AMD_SCENARIO_CACHE", 1) != 0;
    // generator workgroups of a WorkList fill launch (scenario_ring.h: ring_fill_jobs_kernel), at least one
    fill_queue_wgs = env_int("CROWDNAV_AMD_FILL_QUEUE_WGS", 1024);
    if (fill_queue_wgs < 1) fill_queue_wgs = 1;
}

// The ring's device buffers (those a mode or a generator family does not use are 1-element placeholders), its side streams and
// events.  Before the engine uploads its state view; the caller destroys the engine if this fails.
inline int ScenarioRing::create(cn_engine* e) {
    const cn::Params& P = e->P;
    const size_t n = (size_t)P.B * P.A, slots = (size_t)P.B * P.ring_depth, cache = (size_t)cn::kScenarioCacheMax * P.A;
    const bool work_list = mode == Fill::WorkList;
    int rc = CN_OK;
    cn::StateView& S = e->S;
    if ((rc = dev_alloc(e, &S.ring_pos, n * P.ring_mod)) || (rc = dev_alloc(e, &S.ring_goal, n * P.ring_mod)) ||
        (rc = dev_alloc(e, &S.ring_rv, n * P.ring_mod)) ||
        (rc = dev_alloc(e, &S.ring_mt_key, gen_wave ? (size_t)64 : (size_t)624 * cn::kRedoLanes)) ||
        (rc = dev_alloc(e, &S.redo_list, gen_wave ? (size_t)1 : (size_t)P.B * P.ring_mod)) ||
        (rc = dev_alloc(e, &ep_snap, mode == Fill::Beside ? (size_t)P.B : (size_t)1)) ||
        (rc = dev_alloc(e, &S.redo_count, (size_t)2)) ||
        (rc = dev_alloc(e, &S.ring_vel0, first_step ? n * P.ring_mod : (size_t)1)) ||
        (rc = dev_alloc(e, &S.ring_vel0_ok, first_step ? (size_t)P.B * P.ring_mod : (size_t)1)) ||
        (rc = dev_alloc(e, &S.first_list, first_step ? (size_t)P.B * P.ring_mod : (size_t)1)) ||
        (rc = dev_alloc(e, &S.fresh_counts, (size_t)2)) ||
        (rc = dev_alloc(e, &S.ring_filled_in, (size_t)P.B)) || (rc = dev_alloc(e, &S.ring_filled_out, (size_t)P.B)) ||
        (rc = dev_alloc(e, &S.ring_ready, work_list ? slots : (size_t)1)) ||
        (rc = dev_alloc(e, &S.ring_claim, work_list ? slots : (size_t)1)) ||
        (rc = dev_alloc(e, &fill_list, work_list ? (size_t)kFillStreams * (2 + 2 * slots) : (size_t)2)) ||
        (rc = dev_alloc(e, &S.cache_pos, gen_wave ? cache : (size_t)1)) ||
        (rc = dev_alloc(e, &S.cache_goal, gen_wave ? cache : (size_t)1)) ||
        (rc = dev_alloc(e, &S.cache_rv, gen_wave ? cache : (size_t)1)) ||
        (rc = dev_alloc(e, &S.cache_state, (size_t)cn::kScenarioCacheMax)))
        return rc;
    if (work_list) {
        bool ok = hipEventCreateWithFlags(&rollout_done, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < kFillStreams; ++i)
            ok = hipStreamCreateWithFlags(&fill_streams[i], hipStreamNonBlocking) == hipSuccess;
        if (!ok) return fail(CN_ERR_HIP, "cn_create: side streams for the asynchronous scenario fill");
    }
    if (mode == Fill::Beside) {
        // lowest priority: the launch it runs beside becomes ready at the same moment and must get the chip first; the fill's
        // waves take the slots that launch leaves or gives back
        int least = 0, greatest = 0;
        if (hipEventCreateWithFlags(&rollout_done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&fill_done, hipEventDisableTiming) != hipSuccess ||
            hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
            hipStreamCreateWithPriority(&fill_streams[0], hipStreamNonBlocking, least) != hipSuccess)
            return fail(CN_ERR_HIP, "cn_create: side stream for the lagged scenario fill");
    }
    return CN_OK;
}

// waits for the side streams (none with the fills in front); the first error, all streams waited for
static inline hipError_t sync_fill_streams(const ScenarioRing& ring) {
    hipError_t first = hipSuccess;
    for (hipStream_t fs : ring.fill_streams)
        if (fs) {
            const hipError_t err = hipStreamSynchronize(fs);
            if (first == hipSuccess) first = err;
        }
    return first;
}

// (the device buffers are the engine's slabs)
inline void ScenarioRing::destroy() {
    (void)sync_fill_streams(*this);
    for (hipStream_t fs : fill_streams)
        if (fs) (void)hipStreamDestroy(fs);
    if (rollout_done) (void)hipEventDestroy(rollout_done);
    if (fill_done) (void)hipEventDestroy(fill_done);
}

// Fill kernels still in flight on the side streams read the device copy of the io block, the caller's buffers behind it and
// the claim / ready flags (WorkList), or the io block and the envs' episode words (Beside).  Before any of those change hands
// (a new io block, a restart of the bookkeeping: cn_sync, upload_io, cn_rollout_begin) the host waits for them: a straggler of
// the previous rollout must not publish a scenario of the old seed numbering into the new one's ring, nor read buffers the
// caller is about to free.  Once a fill beside a launch has been waited for, its levels are the ring's.
inline int ScenarioRing::drain(cn_engine* e) {
    CN_HIP(sync_fill_streams(*this));
    if (plan.settle()) swap_levels(e->S);
    return CN_OK;
}

// Who must settle: every entry point that reads or writes env state from OUTSIDE a rollout — cn_set_state, cn_get_state,
// cn_reset, cn_step — before it enqueues anything: a fill beside the previous launch reads the envs' episode words and may
// still be running.  Nothing to wait for unless one is out.  (The rollout entry points do not: around_launch takes the levels.)
inline int ScenarioRing::settle(cn_engine* e) { return plan.pending ? drain(e) : CN_OK; }

// Who must forget: every entry point that changes what a solved first step was computed from other than the slot's own scenario —
// the robot's captured simulator (cn_set_robot_sim, cn_drop_robot_sim, cn_drop_sims) or the env state it would be captured from
// (cn_set_state, cn_reset), and cn_rollout_begin — behind its settle, on the engine's stream.  The slots stay unsolved until a
// fill generates into them again: an episode that starts from one redoes its first step as before.
inline int ScenarioRing::forget_first_steps(cn_engine* e) {
    if (!first_step) return CN_OK;
    CN_HIP(hipMemsetAsync(e->S.ring_vel0_ok, 0, (size_t)e->P.B * e->P.ring_mod, e->stream));
    return CN_OK;
}

// cn_rollout_begin, behind its drain and its upload of the io block: an empty scenario cache, every env's first scenario,
// nothing known about the ring.
inline int ScenarioRing::begin(cn_engine* e, uint32_t seed_mod) {
    const cn::RolloutView R{e->io_dev, e->discount, e->discount_len};
    // scenario cache (scenario_ring.h: cached_scenario_wave): on for the wave generators when the episode seeds come from a small
    // set; a new rollout may number its seeds differently, so it starts empty
    e->S.cache_n = (gen_wave && scenario_cache && seed_mod <= (uint32_t)cn::kScenarioCacheMax) ? (int)seed_mod : 0;
    if (gen_wave) {
        CN_HIP(hipMemsetAsync(e->S.cache_state, 0, sizeof(int) * cn::kScenarioCacheMax, e->stream));
        hipLaunchKernelGGL(cn::rollout_begin_wave_kernel, dim3(e->P.B), dim3(cn::kWave), 0, e->stream, e->P, e->C, e->S, R);
    } else {
        hipLaunchKernelGGL(cn::rollout_begin_kernel, dim3(grid_lanes(e)), dim3(cn::kWave), 0, e->stream, e->P, e->C, e->S, R);
    }
    CN_HIP(hipGetLastError());
    plan.begin();
    return CN_OK;
}

// n_steps >= 1 transitions of every env on a ring that cannot run dry under them: launch(R, levels) enqueues the transition
// kernel(s) on the engine's stream, with `levels` as their ring_filled_in argument, and counts them.
// An env consumes at most one ring scenario per transition, so after a fill the next ring_depth transitions cannot run it dry:
// launches inside that budget skip the fill kernels altogether (a 20-step cn_rollout call used to spend more time here than in
// its transitions).  Which calls fill, and whether in front of their launch or beside it, is fill_plan.h's rule.
template <class Launch>
int ScenarioRing::around_launch(cn_engine* e, int n_steps, Launch&& launch) {
    const cn::RolloutView R{e->io_dev, e->discount, e->discount_len};
    cn::FillPlan::Decision plan_says{false, false, false};
    if (mode == Fill::WorkList) {
        // a fill launch per transition launch, on the next side stream, ordered after the PREVIOUS transition kernel (whose
        // episode counters it reads) and beside the one about to be launched; nobody waits for it
        const int this_stream = next_fill_stream;
        hipStream_t fs = fill_streams[this_stream];
        next_fill_stream = (next_fill_stream + 1) % kFillStreams;
        CN_HIP(hipEventRecord(rollout_done, e->stream));
        CN_HIP(hipStreamWaitEvent(fs, rollout_done, 0));
        // scan + persistent generator workgroups on a job list (scenario_ring.h).  (Tried and dropped: 4 workgroups per env walking
        // its slots in order — 4.0 M instead of 20.8 M env-steps/s at the reference geometry, a workgroup stuck on a hard scenario
        // delays its env's later slots; and, rounds 2-5, one workgroup per (env, slot): profiles/HISTORY.md.  Round 2's first
        // attempt at this pair of kernels "hung on the GPU box"; round 6 found why — a generator loop of the shape `for (;;) {
        // lane 0 pops with atomicAdd; j = readfirstlane; if (j >= jobs) break; generate }` never terminates as compiled, so the
        // popping loop of ring_fill_jobs_kernel is written around a ballot instead.)
        int* list = fill_list + (size_t)this_stream * (2 + 2 * (size_t)e->P.B * e->P.ring_depth);
        CN_HIP(hipMemsetAsync(list, 0, 2 * sizeof(int), fs));
        const int items = e->P.B * e->P.ring_depth;
        hipLaunchKernelGGL(cn::ring_fill_scan_kernel, dim3((items + 255) / 256), dim3(256), 0, fs, e->P, e->S, R, list);
        hipLaunchKernelGGL(cn::ring_fill_jobs_kernel, dim3(fill_queue_wgs), dim3(cn::kWave), 0, fs, e->P, e->C, e->S, R, list);
        e->launch_counts[CN_COUNT_ASYNC_FILLS] += 1;
    } else {
        plan_says = plan.call(n_steps);
    }
    const int fill_lanes = e->P.B * e->P.ring_mod;
    const dim3 fill_grid((fill_lanes + cn::kWave - 1) / cn::kWave), redo_grid(cn::kRedoLanes / cn::kWave);
    const int fs_flag = first_step ? 1 : 0;
    // behind ring_redo_kernel, in front of whatever waits for the fill.  In front of the launch the robot's simulator is what the
    // launch's prologue will find or capture (the kernel follows load_robot_view's rule on the same data); beside a launch only
    // once it is known to be captured — else that launch may be the one that captures, and the slots stay unsolved
    const auto solve_first_steps = [&](hipStream_t on) {
        hipLaunchKernelGGL(cn::ring_first_step_kernel, dim3(cn::kFirstStepWgs), dim3(cn::kWave), e->smem, on, e->P, e->S);
        first_step_kernels += 1;
    };
    if (plan_says.take_levels) {  // the fill that ran beside the previous launch: this launch waits for it and takes its levels
        CN_HIP(hipStreamWaitEvent(e->stream, fill_done, 0));
        swap_levels(e->S);
    }
    if (plan_says.sync_fill) {
        if (gen_wave) {
            hipLaunchKernelGGL(cn::ring_fill_wave_kernel, dim3(fill_lanes), dim3(cn::kWave), 0, e->stream, e->P, e->C, e->S, R);
        } else {
            CN_HIP(hipMemsetAsync(e->S.redo_count, 0, 2 * sizeof(int), e->stream));
            hipLaunchKernelGGL(cn::ring_fill_kernel, fill_grid, dim3(cn::kWave), 0, e->stream, e->P, e->C, e->S, R, nullptr, fs_flag);
            hipLaunchKernelGGL(cn::ring_redo_kernel, redo_grid, dim3(cn::kWave), 0, e->stream, e->P, e->C, e->S, fs_flag);
            if (first_step) solve_first_steps(e->stream);
        }
        swap_levels(e->S);
        e->launch_counts[CN_COUNT_RING_FILLS] += 1;
    }
    // a fill beside the launch is ordered behind everything in front of it (the previous launch's episode words, the levels a
    // fill in front just wrote) and enqueued behind it
    if (plan_says.lagged_fill) CN_HIP(hipEventRecord(rollout_done, e->stream));
    const bool sim_known_before = robot_sim_known;
    launch(R, (const int*)e->S.ring_filled_in);
    CN_HIP(hipGetLastError());
    if (e->P.robot_orca) robot_sim_known = true;  // (CN_STORE_EPISODE: every launch of an ORCA robot leaves every env's simulator captured)
    if (plan_says.lagged_fill) {
        // it reads ring_filled_in, as the launch does, and writes ring_filled_out and ring slots of ordinals >= the level the
        // launch was given
        hipStream_t fs = fill_streams[0];
        CN_HIP(hipStreamWaitEvent(fs, rollout_done, 0));
        hipLaunchKernelGGL(cn::ring_fill_begin_kernel, dim3(grid_lanes(e)), dim3(cn::kWave), 0, fs, e->P.B, e->S.ep_word, ep_snap,
                           e->S.redo_count);
        hipLaunchKernelGGL(cn::ring_fill_kernel, fill_grid, dim3(cn::kWave), 0, fs, e->P, e->C, e->S, R, (const int*)ep_snap, fs_flag);
        hipLaunchKernelGGL(cn::ring_redo_kernel, redo_grid, dim3(cn::kWave), 0, fs, e->P, e->C, e->S, fs_flag);
        if (first_step && sim_known_before) solve_first_steps(fs);
        CN_HIP(hipEventRecord(fill_done, fs));
        e->launch_counts[CN_COUNT_RING_FILLS] += 1;
        lagged_fills += 1;
    }
    return CN_OK;
}
