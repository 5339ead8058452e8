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

template <bool UNI>
__global__ __launch_bounds__(kWave) void lookahead_modes_kernel(CvParams P, const double* action_table, ModesParams Q) {
    extern __shared__ double2 modes_lds[];
    const int lane = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)P.chunks), chunk = (int)(blockIdx.x - (unsigned)b * (unsigned)P.chunks);
    const int k = chunk * kWave + lane;
    const int H = P.A - 1, M = Q.M, MH = M * H;
    const size_t g0 = (size_t)b * (size_t)P.A;  // the env's robot row
    double2* const h_pos = modes_lds;           // [2][MH] position before the step in [t & 1], after it in [(t + 1) & 1]
    double2* const h_vel = modes_lds + 2 * MH;  // [2][MH] the velocity a human has, likewise
    double* const h_rad = reinterpret_cast<double*>(modes_lds + 4 * MH);  // [H]

    // the env's velocity rows [M][n_steps][H]; row r = m H + h of step t lies at (m n_steps + t) H + h
    const double2* const vel_rows = reinterpret_cast<const double2*>(Q.human_vel) + (size_t)b * (size_t)M * (size_t)P.n_steps * (size_t)H;
    for (int r = lane; r < MH; r += kWave) {  // every mode starts from the humans as env b holds them
        const int h = r % H;
        h_pos[r] = P.pos[g0 + 1 + h], h_vel[r] = P.vel[g0 + 1 + h];
    }
    if (lane < H) h_rad[lane] = P.rv[g0 + 1 + lane].x;
    // the owner's first row: where its table rows start (a lane >= MH forms no address from it)
    const int m0 = lane / H;
    const size_t off0 = (size_t)m0 * (size_t)P.n_steps * (size_t)H + (size_t)(lane - m0 * H);

    // this lane's branch: the robot as env b holds it, a fresh book per mode
    const bool mine = k < P.K;
    const size_t v_env = (size_t)b * (size_t)P.K + (size_t)(mine ? k : 0);  // (a tail lane forms no address of its own)
    double px = 0.0, py = 0.0, gx = 0.0, gy = 0.0, rad = 0.0, theta = 0.0, gtime = 0.0;
    if (mine) {
        const double2 p = P.pos[g0], g = P.goal[g0], rv = P.rv[g0];
        px = p.x, py = p.y, gx = g.x, gy = g.y, rad = rv.x;
        gtime = P.gtime[b];
        theta = P.theta[b];  // (carried by UNI engines only)
    }
    unsigned running = mine ? (1u << M) - 1u : 0u;  // bit m: mode m of this branch has not ended
    double m_ret[kModesMax], m_time[kModesMax];
    int m_steps[kModesMax], m_info[kModesMax];
#pragma unroll
    for (int m = 0; m < kModesMax; ++m) m_ret[m] = 0.0, m_time[m] = 0.0, m_steps[m] = 0, m_info[m] = CN_NOTHING;
    const double2* const row = reinterpret_cast<const double2*>(action_table) + v_env * (size_t)P.n_steps;
    __syncthreads();

    for (int t = 0; t < P.n_steps; ++t) {
        const double2* const cur = h_pos + (t & 1) * MH;
        double2* const nxt = h_pos + ((t + 1) & 1) * MH;
        const double2* const vcur = h_vel + (t & 1) * MH;
        double2* const vnxt = h_vel + ((t + 1) & 1) * MH;
        double2 v0 = make_double2(0.0, 0.0);
        if (lane < MH) v0 = vel_rows[off0 + (size_t)t * (size_t)H];  // the velocity this lane's first human chooses at step t
        if (running) {
            const double2 a = row[t];
            const RobotStep rs = robot_step(UNI, px, py, a.x, a.y, theta, P.dt);  // once per lane and step (transition.h)
            const bool reaching = norm2(rs.ex - gx, rs.ey - gy) < rad;
            const bool timeout = gtime >= P.time_limit - 1.0;
            const double disc = (t < kMaxDiscount && t < P.discount_len) ? P.discount[t] : 0.0;
            gtime += P.dt;  // the clock after this step, which a mode ending here reports
            const bool last = t == P.n_steps - 1;
#pragma unroll
            for (int m = 0; m < kModesMax; ++m) {
                if (m < M && (running >> m & 1u)) {
                    // slot order scan over the swept distances of mode m and its outcome (transition.h)
                    const double2* const mp = cur + m * H;
                    const double2* const mv = vcur + m * H;
                    double dmin = std::numeric_limits<double>::infinity();
                    bool collision = false;
                    for (int i = 0; i < H; ++i) {
                        const double2 hp = mp[i], hv = mv[i];
                        const double2 cp = closest_point(hp.x - px, hp.y - py, hv.x - rs.vx, hv.y - rs.vy, P.dt);
                        const double c = norm2(cp.x, cp.y) - h_rad[i] - rad;
                        dmin = scan_dmin(dmin, collision, c);
                        collision = scan_collision(collision, c);
                    }
                    const Outcome o = outcome_of(timeout, collision, reaching, dmin, P.success_reward, P.collision_penalty,
                                                 P.discomfort_dist, P.discomfort_factor, P.dt);
                    // the mode's book (CN_BOOK_TRANSITION; a running mode has made t transitions)
                    m_ret[m] = m_ret[m] + disc * o.reward;
                    m_info[m] = o.info;
                    m_steps[m] = t + 1;
                    m_time[m] = gtime;
                    if (o.done || last) running &= ~(1u << m);
                }
            }
            // Agent.step
            px = rs.ex, py = rs.ey;
            theta = robot_after(UNI, a.x, rs.th, rs.vx, rs.vy, theta).theta;
        }
        // the humans' move of this step, by the lane that owns each row: one multiply and one add per coordinate
        if (lane < MH) {
            const double2 p = cur[lane];
            nxt[lane] = make_double2(p.x + v0.x * P.dt, p.y + v0.y * P.dt);
            vnxt[lane] = v0;
        }
        for (int r = lane + kWave; r < MH; r += kWave) {
            const int m = r / H;
            const double2 v = vel_rows[((size_t)m * (size_t)P.n_steps + (size_t)t) * (size_t)H + (size_t)(r - m * H)];
            const double2 p = cur[r];
            nxt[r] = make_double2(p.x + v.x * P.dt, p.y + v.y * P.dt);
            vnxt[r] = v;
        }
        if (!__syncthreads_or(running ? 1 : 0)) break;  // ... and nxt / vnxt are written
    }

    if (mine) {
        // the reduction (header): float64, every product and sum a separate operation, sequential in m from 0.0
        const double w_all = 1.0 / (double)M;
        double mean = 0.0, risk = 0.0, worst_ret = m_ret[0], worst_time = m_time[0];
        int worst = 0, worst_info = m_info[0], worst_steps = m_steps[0];
#pragma unroll
        for (int m = 0; m < kModesMax; ++m) {
            if (m < M) {
                const double w = Q.weight ? Q.weight[(size_t)b * (size_t)M + m] : w_all;
                mean = mean + w * m_ret[m];
                risk = risk + w * (m_info[m] == CN_COLLISION ? 1.0 : 0.0);
                if (m_ret[m] < worst_ret) worst = m, worst_ret = m_ret[m], worst_info = m_info[m], worst_steps = m_steps[m], worst_time = m_time[m];
                const size_t at = v_env * (size_t)M + m;
                if (Q.out.ret) Q.out.ret[at] = m_ret[m];
                if (Q.out.info) Q.out.info[at] = (uint8_t)m_info[m];
                if (Q.out.steps) Q.out.steps[at] = m_steps[m];
                if (Q.out.time) Q.out.time[at] = m_time[m];
            }
        }
        const double r = Q.reduce == CN_MODES_MIN ? worst_ret : mean;
        Q.out.score[v_env] = r - Q.risk_penalty * risk;
        if (Q.out.risk) Q.out.risk[v_env] = risk;
        if (Q.out.worst_mode) Q.out.worst_mode[v_env] = worst;
        if (Q.out.worst_info) Q.out.worst_info[v_env] = (uint8_t)worst_info;
        if (Q.out.worst_steps) Q.out.worst_steps[v_env] = worst_steps;
        if (Q.out.worst_time) Q.out.worst_time[v_env] = worst_time;
    }
}

}  // namespace cn
