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
    const Smem s = carve<MAXL>(P);
    const Lane L = lane_of(P);
    AgentRegs r = {};
    if (L.valid) load_agent(S, L.gi, r);
    // the robot's simulator is never solved; its pairs (build_pairs gives the robot lane every human) read finite radii
    if (L.lane < P.nA) s.rview[L.lane] = (float)(r.rad + 0.01 + P.robot_safety);
    build_pairs(P, s);
    if (KD) kd_fresh(P, s, L);
    const bool human = L.valid && L.a > 0;
    // row (b, mode, t, h): B n_modes n_steps (A - 1) is within an int (the host checks), the index is formed in size_t
    double2* row = human_vel + (((size_t)(human ? L.env : 0) * n_modes + mode) * n_steps) * P.NC + (human ? L.a - 1 : 0);
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
