// cn_lookahead_actions under CN_HUMANS_CONSTANT_VELOCITY (include/crowdnav_amd.h, "Lookahead human model"): branch (b, k) is
// step_core's transition (step_kernels.h) with ONE substitution — the velocity a human "chooses" is its own current float64
// velocity — so a branch needs no ORCA, no exchange between agents, and the humans' trajectory is the same for all K branches of
// an env.  Hence another decomposition than rollout_lookahead_kernel's wave-per-branch:
//   lane = branch.  A 64-lane workgroup (one wave) holds 64 consecutive branches k of ONE env b; K > 64 takes several
//     workgroups per env, the last with a tail.  The robot's position, heading, time and book live in the lane's registers.
//   humans = shared.  Lane h < H loads human h's row once and keeps it in registers, where it advances it by the sequential
//     rule p <- p + v dt; every step it leaves the NEXT position in LDS (two position buffers, so one barrier per step — the
//     __syncthreads_or that also decides whether the wave has a running lane left).  All lanes read a human at the same LDS
//     address: broadcast reads.  Human counts 1..63 and the parked placeholders of the `mixed` rule run the same code.
//   action table [B][K][n][2]: read where it lies, one 16-byte load per lane and step from the lane's own contiguous row; only
//     a running lane loads, so rows after a branch's end are not read.  (Staging the wave's block through LDS, 8 steps of
//     coalesced 128-byte row segments at a time, was built and measured: 0.108 ms against 0.088 ms per call at 4096 envs, K = 64,
//     n = 12 — profiles/lookahead_cv_timing.txt.)
//   outputs through the device copy of the caller's cn_lookahead_out.  final_state8 (when asked for) is written by the lane at
//     the step its branch ends — the human rows are those of that step, which the LDS holds then and not later.
// Compiled with the translation unit's flags: -ffp-contract=off keeps every product and sum below a separate IEEE operation,
// the one fused multiply-add is norm2's (tests/lookahead_cv_reference.py restates it).
#pragma once
#include "step_kernels.h"

namespace cn {

struct CvParams {
    int B, K, A, n_steps;  // envs, candidates per env, agents per env (robot + humans), horizon
    int chunks;            // workgroups per env = ceil(K / 64)
    int discount_len;
    double dt, time_limit, success_reward, collision_penalty, discomfort_dist, discomfort_factor;
    const double2 *pos, *vel, *goal, *rv;  // the engine's state, [B][A]; read only
    const double *gtime, *theta;           // [B]
    const double* discount;                // cn_set_gamma's table
};

constexpr int kCvHumans = 63;  // check_config: num_humans <= 63

// Both kernels' body is lookahead_cv_body.inc: the decomposition above around transition.h's functions, with the compile-time
// flag PATHS choosing where a human's velocity comes from and GOAL whether ret carries the goal-progress term.
template <bool UNI>
__global__ __launch_bounds__(kWave) void lookahead_cv_kernel(CvParams P, const double* action_table, const cn_lookahead_out* Od) {
    constexpr bool PATHS = false, GOAL = false;
    const double* const human_vel = nullptr;
    const double goal_weight = 0.0;
#include "lookahead_cv_body.inc"
}

// cn_lookahead_paths: the same lane body with the humans' velocities read from the caller's table.
// human_vel: [B][n_steps][A - 1][2] float64, the velocity every human takes at every step of the horizon
template <bool UNI>
__global__ __launch_bounds__(kWave) void lookahead_paths_kernel(CvParams P, const double* action_table, const double* human_vel,
                                                                const cn_lookahead_out* Od) {
    constexpr bool PATHS = true, GOAL = false;
    const double goal_weight = 0.0;
#include "lookahead_cv_body.inc"
}

// The goal forms of the two (cn_lookahead_set_goal_weight with a weight != 0): the same lane body under GOAL = true, the
// engine's weight as one more kernel argument.  Kernels of their own, so that the two above keep their instructions and a
// weight of 0.0 launches what it always launched.
template <bool UNI>
__global__ __launch_bounds__(kWave) void lookahead_cv_goal_kernel(CvParams P, const double* action_table, const cn_lookahead_out* Od,
                                                                  double goal_weight) {
    constexpr bool PATHS = false, GOAL = true;
    const double* const human_vel = nullptr;
#include "lookahead_cv_body.inc"
}

template <bool UNI>
__global__ __launch_bounds__(kWave) void lookahead_paths_goal_kernel(CvParams P, const double* action_table, const double* human_vel,
                                                                     const cn_lookahead_out* Od, double goal_weight) {
    constexpr bool PATHS = true, GOAL = true;
#include "lookahead_cv_body.inc"
}

}  // namespace cn
