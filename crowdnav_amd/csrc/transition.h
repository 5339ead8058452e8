// The transition of CrowdSim.step (crowd_sim.py:317-420, update or onestep_lookahead alike), stated once for every kernel that
// makes it.  lookahead_cv_body.inc and lookahead_modes_kernel.h take all of it; step_core (step_kernels.h), swept_distance
// (rollout_fused.h) and sarl_reward_of (sarl_kernels.h) take closest_point.
//
// One step of one env, the robot against every human in slot order:
//   robot action   holonomic: the action row IS the velocity (vx, vy).  Unicycle ActionRot(v, r): the collision test uses
//                  v (cos, sin)(r + theta) (crowd_sim.py:339-341); the end point is compute_position's, px + cos(theta + r) v dt
//                  (agent.py:115-118); after the step theta = (theta + r) % 2 pi — python's %, the sign of the divisor — and the
//                  velocity v (cos, sin)(theta) (agent.py:127-135).
//   swept distance the human's CURRENT velocity against the robot's NEW action over the step: with (x1, y1) the human seen from
//                  the robot and (wx, wy) the relative velocity, point_to_segment_dist(x1, y1, x1 + wx dt, y1 + wy dt, 0, 0)
//                  (utils.py:4-26, its zero-length segment included) minus both radii (crowd_sim.py:331-351).
//   scan           dmin is the minimum of the distances seen BEFORE the first negative one: the reference breaks out of its loop
//                  at the first collision (crowd_sim.py:343-351).
//   outcome        Timeout (global_time >= time_limit - 1) > Collision > ReachGoal (end point within the robot's radius of its
//                  goal) > Danger (dmin < discomfort_dist: (dmin - discomfort_dist) discomfort_factor dt) > Nothing
//                  (crowd_sim.py:364-389); the first three end the episode.
//
// Every function is a leaf on scalars — no parameter block, no LDS, no pointer: a kernel hands in what it holds in registers and
// keeps its own loads, barriers and loop shape, so a caller's instruction stream depends on the arithmetic alone (the lane body
// as ONE function over the parameter block did change the kernels: profiles/lookahead_paths_kernels.txt).  The translation
// units compile with -ffp-contract=off: every product and sum below is its own IEEE operation, in the order written; norm2's
// fma (scenario_device.h) is the one fused operation.  The routes are compared bit for bit (tests/test_transition_routes.py
// and the _same_bits suites).  A change of the rule is made here AND in the text that still mirrors it: the robot's action,
// scan and ladder of step_core, reduce_env's branch-free scan and ladder, sarl_reward_of's scan with break, ladder and end point.
#pragma once
#include "../../include/crowdnav_amd.h"
#include "scenario_device.h"  // norm2

namespace cn {

__device__ __forceinline__ double python_fmod(double x, double y) {  // python's float %: result takes the sign of y
    double m = fmod(x, y);
    if (m != 0.0 && ((m < 0.0) != (y < 0.0))) m += y;
    return m;
}

// The point of the segment (x1, y1) -> (x1 + wx dt, y1 + wy dt) closest to the origin (utils.py:4-26).  A zero-length segment
// makes u NaN; the select discards it (utils.py:11-13).
__device__ __forceinline__ double2 closest_point(double x1, double y1, double wx, double wy, double dt) {
    const double x2 = x1 + wx * dt, y2 = y1 + wy * dt;
    const double sx = x2 - x1, sy = y2 - y1;
    double u = ((0.0 - x1) * sx + (0.0 - y1) * sy) / (sx * sx + sy * sy);
    u = (u > 1.0) ? 1.0 : ((u < 0.0) ? 0.0 : u);
    const bool degenerate = (sx == 0.0 && sy == 0.0);
    return make_double2(degenerate ? 0.0 - x1 : (x1 + u * sx) - 0.0, degenerate ? 0.0 - y1 : (y1 + u * sy) - 0.0);
}

// One step of the slot-order scan over the boundary distances c: first the minimum, then the flag.
__device__ __forceinline__ double scan_dmin(double dmin, bool collision, double c) {
    return (!collision && !(c < 0.0) && c < dmin) ? c : dmin;
}
__device__ __forceinline__ bool scan_collision(bool collision, double c) { return collision || c < 0.0; }

struct Outcome { double reward; int info; bool done; };
__device__ __forceinline__ Outcome outcome_of(bool timeout, bool collision, bool reaching, double dmin, double success_reward,
                                              double collision_penalty, double discomfort_dist, double discomfort_factor, double dt) {
    if (timeout) return Outcome{0.0, CN_TIMEOUT, true};
    if (collision) return Outcome{collision_penalty, CN_COLLISION, true};
    if (reaching) return Outcome{success_reward, CN_REACH_GOAL, true};
    if (dmin < discomfort_dist) return Outcome{(dmin - discomfort_dist) * discomfort_factor * dt, CN_DANGER, false};
    return Outcome{0.0, CN_NOTHING, false};
}

// The robot's step.  (a0, a1) is the action row: (vx, vy), or ActionRot(v, r) of a unicycle.  vx, vy: the velocity the swept
// test is made with; ex, ey: where the step ends; th: theta + r (unicycle).
struct RobotStep { double vx, vy, ex, ey, th; };
__device__ __forceinline__ RobotStep robot_step(bool unicycle, double px, double py, double a0, double a1, double theta, double dt) {
    RobotStep s{a0, a1, 0.0, 0.0, 0.0};
    if (unicycle) {
        s.th = theta + a1;
        s.vx = a0 * cos(a1 + theta), s.vy = a0 * sin(a1 + theta);
    }
    s.ex = px + s.vx * dt, s.ey = py + s.vy * dt;
    if (unicycle) s.ex = px + cos(s.th) * a0 * dt, s.ey = py + sin(s.th) * a0 * dt;
    return s;
}
// ... and what the robot holds after it (Agent.step): velocity and heading.  Holonomic: the action, the heading as it was.
struct RobotAfter { double vx, vy, theta; };
__device__ __forceinline__ RobotAfter robot_after(bool unicycle, double v, double th, double vx, double vy, double theta) {
    if (!unicycle) return RobotAfter{vx, vy, theta};
    const double theta1 = python_fmod(th, 2 * 3.141592653589793);
    return RobotAfter{v * cos(theta1), v * sin(theta1), theta1};
}

}  // namespace cn
