// cn_predict_orca: the table of human velocities that ORCA among the humans gives, the robot unseen — n steps of every env's
// humans from the engine's state as it stands, in one launch, with the step kernels' own ORCA code.
//
// The workgroup is step_kernel's (Params, carve, lane_of, build_pairs: E whole envs, agents = lanes of wave 0, the pair
// phases over every wave) under a by-value copy of Params in which robot_visible = 0 and robot_orca = 0 (the host makes it):
// the humans' candidate lists then hold the other humans only, and the robot lane solves nothing.  Per step: orca_phases for
// the human lanes, Agent.step's move (step_core's: p + v dt in float64, product and sum separate), one 16-byte store of the
// lane's velocity row.  What step_core does for the robot — the action, the swept test with its two barriers, the reward — is
// not here: nothing of it feeds the humans when they do not see the robot.
//
// The simulators are fresh ones (cn_drop_sims): on the kd route the visiting order starts as kd_identity_row's and is carried
// in LDS through the n steps; the engine's kd_order / kd_valid rows are neither read nor written, and nothing else of the
// engine is written either.
//
// cn_predict_orca_robot (ROBOT = true): the same steps with the robot in the humans' sight, following a table of actions the
// caller gives — the host's copy of Params has robot_visible = 1 (robot_orca = 0 as before), so candidate lists, pair
// descriptors and the kd identity rows hold the robot exactly as step_kernel has them on a robot_visible = 1 CN_ROBOT_EXTERNAL
// engine.  Order of events within step t, CrowdSim.step's: the humans solve against the robot where it stands and with the
// velocity it has (orca_phases stages every agent lane's registers, the robot's among them, as float32(radius + 0.01 +
// human_safety) like any other agent of a human's simulator); the humans move; the robot lane takes row t of its table through
// robot_step / robot_after (transition.h).  The robot has no swept test, reward, done or time: all n rows are followed.  The
// row is requested before orca_phases, so its latency hides behind the solve, and there is no further barrier: the robot lane
// only rewrites its own registers, which the next step's stage phase publishes behind the loop's one block_sync.
// The flag lives on the shared body text (predict_orca_body.inc), not on predict_orca_kernel's template list: a third template
// argument would rename the robot-unseen kernels, and with ROBOT = false the body is the text above and nothing else.
#pragma once
#include "step_kernels.h"

namespace cn {

// kd_load for simulators that have just been built, without the engine's rows
__device__ __forceinline__ void kd_fresh(const Params& P, const Smem& s, const Lane& L) {
    const KdSmem k = kd_view(P, s);
    if (L.lane < P.nA) kd_identity_row(k.ord + (size_t)L.lane * k.row, k.row, P.A, L.a, P.robot_visible);
    if (threadIdx.x == 0) *k.gen = 0;
    for (int i = threadIdx.x; i < P.E * 2 * 2; i += P.threads) k.count[i] = 0;  // no "last step's tree" yet
}

// human_vel: [B][n_modes][n_steps][A - 1] double2; slot `mode` is written, every row of it, and no other
template <int MAXL, bool KD>
__global__ __launch_bounds__(kMaxBlock) void predict_orca_kernel(Params P, StateView S, int n_steps, int n_modes, int mode,
                                                                 double2* human_vel) {
    constexpr bool ROBOT = false, UNI = false;
    constexpr const double* robot_actions = nullptr;
    constexpr long long env_stride = 0;
#include "predict_orca_body.inc"
}

// ... with the robot in sight: robot_actions row (b, t) at robot_actions + 2 (b env_stride + t); UNI: the rows are
// ActionRot(v, r), the heading S.theta's
template <int MAXL, bool KD, bool UNI>
__global__ __launch_bounds__(kMaxBlock) void predict_orca_robot_kernel(Params P, StateView S, int n_steps, int n_modes, int mode,
                                                                       double2* human_vel, const double* robot_actions,
                                                                       long long env_stride) {
    constexpr bool ROBOT = true;
#include "predict_orca_body.inc"
}

}  // namespace cn
