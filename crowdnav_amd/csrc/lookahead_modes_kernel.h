// cn_lookahead_modes (include/crowdnav_amd.h, "Lookahead under several predicted futures"): branch (b, k) of
// cn_lookahead_paths scored against M tables of predicted human velocities at once, and the M returns reduced in the lane.
// The robot of a branch does not depend on the humans — its actions are open-loop — so the decomposition of
// lookahead_cv_kernel.h stays (lane = branch, a 64-lane workgroup = 64 consecutive k of ONE env, the env's humans shared through
// LDS) and only what depends on the humans is made M times:
//   once per lane and step   the action row's 16-byte load, the robot's action, end point, reaching test, clock, discount and
//     move.  A lane loads rows while ANY of its modes runs; the workgroup stops when no lane has a running mode (the same
//     __syncthreads_or).
//   once per lane, step and running mode   the slot-order swept scan over that mode's H humans, the dmin rule, the outcome and
//     the mode's book: a running bit, return, info, steps, end time.  The books live in registers: every
//     loop over modes below is fully unrolled over the compile-time cap kModesMax with `m < M` as a uniform guard, so nothing is
//     indexed dynamically and nothing lives in scratch.
// The transition is transition.h's, called in lookahead_cv_body.inc's order with PATHS = true (that file is included text whose
// two kernels are not parametrised further); tests/test_lookahead_modes.py pins it: every mode's ret, info, steps and time are
// bit-equal to cn_lookahead_paths with that mode's table.  Timeout and ReachGoal depend on the robot alone and so end every
// mode still running at that step; a Collision ends its own mode.
//
// Humans.  Row r = m H + h of the workgroup is human slot h + 1 under mode m: M H rows, up to 8 x 63 = 504, more than the 64
// lanes.  Row r is owned by lane r % 64: an owner loops over r = lane, lane + 64, ...  Positions and velocities are
// double-buffered in LDS as h_pos / h_vel are there — what a human has before step t in [t & 1], after it in [(t + 1) & 1] —
// and, unlike there, the owner keeps no copy in registers: it reads its row's position before the step from [t & 1], makes the
// same one multiply and one add, and writes [(t + 1) & 1].  The owner's first row (r = lane, all there is while M H <= 64) has
// its table row loaded at the top of the iteration, so that the load's latency hides behind the scan; further rows are loaded
// where they are used.  Only rows of steps the workgroup makes are loaded.
// The LDS is sized by the launch (4 M H double2 + H radii: 1.3 KB at 4 modes x 5 humans, 32.3 KB at 8 x 63), so that the
// common small crowds keep the registers' occupancy.
// One barrier per step is enough, by lookahead_cv_body.inc's argument restated for looped owners: every row r is written by
// exactly one lane, whichever trip of its loop that is.  The scan of iteration t reads rows of [t & 1]; those were published
// before the barrier of iteration t - 1 (or the first __syncthreads) by their owners, and are next written in iteration t + 1,
// behind the barrier of iteration t, which every scanning lane passes only after its scan.  The owner's own read of [t & 1] in
// iteration t is of a row nobody but itself writes.  Iteration t writes [(t + 1) & 1], which was last read by the scans (and
// owners) of iteration t - 1, all of them in front of the barrier of iteration t - 1.  Nothing leans on the workgroup being a
// single wave, and nothing is read after the loop.
// Compiled with the translation unit's flags (-ffp-contract=off -fno-slp-vectorize); norm2's fma is the one fused operation.
#pragma once
#include "lookahead_cv_kernel.h"

namespace cn {

constexpr int kModesMax = 8;  // cn_path_modes.n_modes: 1 .. 8

struct ModesParams {
    int M, reduce;  // modes per env; CN_MODES_MEAN | CN_MODES_MIN
    double risk_penalty;
    const double* human_vel;  // [B][M][n_steps][A - 1][2]
    const double* weight;     // [B][M] or nullptr = 1.0 / (double)M each
    cn_modes_out out;         // the caller's arrays (device pointers)
};

// dynamic LDS of one workgroup: both position buffers, both velocity buffers, the radii
inline size_t modes_lds_bytes(int M, int H) { return (size_t)4 * (size_t)M * (size_t)H * sizeof(double2) + (size_t)H * sizeof(double); }

// The kernel's body is lookahead_modes_body.inc: included text with the compile-time flag GOAL, for lookahead_cv_body.inc's
// reason.
template <bool UNI>
__global__ __launch_bounds__(kWave) void lookahead_modes_kernel(CvParams P, const double* action_table, ModesParams Q) {
    constexpr bool GOAL = false;
    const double goal_weight = 0.0;
#include "lookahead_modes_body.inc"
}

// Its goal form (cn_lookahead_set_goal_weight with a weight != 0): every mode's return gets the goal-progress term at the step
// that mode ends, ahead of the reduction.  The engine's weight is one more kernel argument; the kernel above keeps its
// instructions.
template <bool UNI>
__global__ __launch_bounds__(kWave) void lookahead_modes_goal_kernel(CvParams P, const double* action_table, ModesParams Q,
                                                                     double goal_weight) {
    constexpr bool GOAL = true;
#include "lookahead_modes_body.inc"
}

}  // namespace cn
