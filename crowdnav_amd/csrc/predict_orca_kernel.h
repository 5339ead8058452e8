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

// cn_predict_orca_goals: predict_orca_kernel's table for M hypotheses about where the humans are heading, side by side in one
// launch.  The workgroup is the same one over B M VIRTUAL envs: the host's copy of Params has B = B M (robot_visible = 0 and
// robot_orca = 0 as above), so lane_of, build_pairs and the grid count virtual envs, and L.env is ve = b M + m.  Two things are
// indexed by it in global memory: the goal of a human lane, one 16-byte load from goals [B][M][A - 1] (row ve (A - 1) + h),
// and the output row (ve n_steps + t) (A - 1) + h of human_vel [B][M][n_steps][A - 1].  The agents themselves are the real
// env's: row (ve / M) A + a of the state — L.gi, which lane_of forms from the virtual env, is NOT a row of the state and is
// not used.  Nothing else of the body reads global memory by env: orca_phases and what it calls (pair phases, kd trees, the
// programs) work on registers and LDS only.  A parked placeholder of the `mixed` rule keeps the goal of its state row (its
// own position), so it gets what predict_orca_kernel gives it.
// A body of its own, not a flag on predict_orca_body.inc: that text is shared so that the two kernels above keep their
// instruction streams, and this kernel differs from it where the agent is loaded and where the row is addressed.
template <int MAXL, bool KD>
__global__ __launch_bounds__(kMaxBlock) void predict_orca_goals_kernel(Params P, StateView S, int n_steps, int n_modes,
                                                                       const double2* goals, double2* human_vel) {
    const Smem s = carve<MAXL>(P);
    const Lane L = lane_of(P);
    AgentRegs r = {};
    if (L.valid) load_agent(S, (size_t)(L.env / n_modes) * P.A + L.a, r);
    if (L.lane < P.nA) s.rview[L.lane] = (float)(r.rad + 0.01 + P.robot_safety);  // (read by the robot lane's pairs, never solved)
    build_pairs(P, s);
    if (KD) kd_fresh(P, s, L);
    const bool human = L.valid && L.a > 0;
    if (human && !is_parked(make_double2(r.px, r.py))) {
        const double2 g = goals[(size_t)L.env * P.NC + (L.a - 1)];
        r.gx = g.x, r.gy = g.y;
    }
    // row (ve, t, h): B M n_steps (A - 1) is within an int (the host checks), the index is formed in size_t
    double2* row = human_vel + ((size_t)(human ? L.env : 0) * n_steps) * P.NC + (human ? L.a - 1 : 0);
    for (int t = 0; t < n_steps; ++t) {
        float vx, vy;
        orca_phases<MAXL, KD>(P, s, L, r, 0.0f, human, vx, vy);
        if (human) {
            const double nvx = vx, nvy = vy;
            r.px = r.px + nvx * P.dt;
            r.py = r.py + nvy * P.dt;
            r.vx = nvx;
            r.vy = nvy;
            row[(size_t)t * P.NC] = make_double2(nvx, nvy);
        }
        block_sync(P);  // the solve's last LDS reads, before the next step's stage phase writes
    }
}

}  // namespace cn
