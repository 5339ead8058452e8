// Device side of the shooting planners (cn_plan_*, plan.hip): the kernels between "score K action sequences per env"
// (cn_lookahead_actions / cn_lookahead_values) and "a robot that plans" — draw the candidates, rank them and update the sampling
// distribution (CEM: refit to the elites; MPPI: softmax-weighted mean), shift the plan behind a real step, seed it with the
// goal-directed prior.  External robots: holonomic ones, rows (vx, vy) clipped to the speed disc; and, once cn_plan_set_unicycle
// has named the rotation bound, unicycle ones, rows (v, r) clipped to the box [0, v_pref] x [-R, R] — kernels of their own
// (the *_uni_kernel forms below), so that no float64 atan2 / cos / sin of the unicycle prior enters a holonomic kernel.
//
// The arithmetic is the header's (include/crowdnav_amd.h, "Device CEM planner" and "Device MPPI update"), one IEEE operation per
// product and sum in the order written there (the library is built with -ffp-contract=off), so that tests/plan_reference.py and
// tests/plan_mppi_reference.py restate it in numpy float64 bit for bit — apart from the draw's log / cos / sin and the MPPI
// weights' exp, which are the device libm's.
//   plan_reset_kernel  lane = (env, t)            the prior: full speed (or what reaches the goal in one step) towards the goal
//   plan_draw_kernel   lane = (env, k, t)         one Philox4x32-10 block -> one Box-Muller pair -> one clipped 16-byte row
//   plan_refit_kernel  workgroup = env, one wave  ranks by counting over the scores in LDS; best row; elite mean / std
//   plan_mppi_kernel   workgroup = env, one wave  the same ranks and best row; weights exp((s - s_max) / T) in LDS; weighted mean / std
//   plan_shift_kernel  lane = (env, component)    walks t upwards in place: row t <- row t + 1, or the prior at an episode start
//   predict_kernel     lane = (env, mode, human)  the table of predicted human velocities the *_paths / *_modes planners score against
//   goal_hypotheses_kernel  lane = (env, mode, human)  the table of hypothesised human goals cn_predict_orca_goals predicts from
// Unicycle forms: plan_draw_uni_kernel and plan_mppi_uni_kernel are the lane bodies above under UNI = true (the clip alone
// differs); plan_reset_uni_kernel is lane = env, because the (v, r) prior is a recurrence in t (position and heading), walked as
// predict_kernel walks to_goal; plan_shift_uni_kernel keeps lane = (env, component) for the shifted envs and hands a re-seeded
// env's recurrence to its component-0 lane.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cn {

constexpr int kPlanMaxCandidates = 1024;  // K: the scores of one env in LDS (8 KiB; the MPPI update holds K weights beside them)
constexpr int kPlanMaxElites = 64;        // E: the elite indices in LDS
constexpr int kPlanBlock = 256;           // lanes per workgroup of the streaming kernels (reset, draw, shift)

struct PlanWords {
    uint32_t w[4];
};

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between rounds
__host__ __device__ inline PlanWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return PlanWords{{c0, c1, c2, c3}};
}

// the goal-directed prior of env b: robot row `r` = b A of the engine state
__device__ inline double2 plan_prior(const double2* pos, const double2* goal, const double2* rv, size_t r, double dt) {
    const double2 p = pos[r], g = goal[r];
    const double dx = g.x - p.x, dy = g.y - p.y;
    const double dist = sqrt(dx * dx + dy * dy);
    const double reach = dist / dt, v_pref = rv[r].y;
    const double speed = v_pref < reach ? v_pref : reach;
    if (!(dist > 0.0)) return make_double2(0.0, 0.0);
    return make_double2((dx / dist) * speed, (dy / dist) * speed);
}

// The (v, r) clip of a unicycle row: the box [0, v_pref] x [-R, R] (no reverse gear)
__device__ inline double2 plan_clip_uni(double2 a, double v_pref, double R) {
    a.x = a.x < 0.0 ? 0.0 : (a.x > v_pref ? v_pref : a.x);
    a.y = a.y < -R ? -R : (a.y > R ? R : a.y);
    return a;
}

// The clip of either robot.  Holonomic: onto the speed disc.
template <bool UNI>
__device__ __forceinline__ double2 plan_clip(double2 a, double v_pref, double R) {
    if (UNI) return plan_clip_uni(a, v_pref, R);
    const double nrm = sqrt(a.x * a.x + a.y * a.y);
    if (nrm > v_pref) {
        const double s = v_pref / nrm;
        a.x *= s, a.y *= s;
    }
    return a;
}

// The goal-directed prior of a unicycle, a recurrence in t: turn towards the goal by at most R, then drive at full speed (or
// what reaches the goal in one step) along the new heading — robot_step's end point, in its operation order.  The turn is
// the bearing's difference to the heading wrapped into [-pi, pi) by explicit operations.
struct PlanUniState {
    double px, py, th;
};
__device__ inline double2 plan_prior_uni_step(PlanUniState& s, double gx, double gy, double v_pref, double dt, double R) {
    const double dx = gx - s.px, dy = gy - s.py;
    const double dist = sqrt(dx * dx + dy * dy);
    const double reach = dist / dt;
    const double speed = v_pref < reach ? v_pref : reach;
    if (!(dist > 0.0)) return make_double2(0.0, 0.0);
    const double bearing = atan2(dy, dx);
    const double d = bearing - s.th;
    const double turn = d - 6.283185307179586 * floor((d + 3.141592653589793) / 6.283185307179586);
    const double r = turn < -R ? -R : (turn > R ? R : turn);
    s.th = s.th + r;
    s.px = s.px + cos(s.th) * speed * dt;
    s.py = s.py + sin(s.th) * speed * dt;
    return make_double2(speed, r);
}
// ... all n rows of env b into mean[b]
__device__ inline void plan_prior_uni(const double2* pos, const double2* goal, const double2* rv, const double* theta, size_t b, int A,
                                      int n, double dt, double R, double2* mean) {
    const size_t r = b * A;
    const double2 p = pos[r], g = goal[r];
    const double v_pref = rv[r].y;
    PlanUniState s{p.x, p.y, theta[b]};
    for (int t = 0; t < n; ++t) mean[b * n + t] = plan_prior_uni_step(s, g.x, g.y, v_pref, dt, R);
}

__global__ __launch_bounds__(kPlanBlock) void plan_reset_kernel(int B, int A, int n, double dt, double init_std, const double2* pos,
                                                                const double2* goal, const double2* rv, const uint8_t* mask,
                                                                double2* mean, double2* std) {
    const size_t i = (size_t)blockIdx.x * kPlanBlock + threadIdx.x;
    if (i >= (size_t)B * n) return;
    const size_t b = i / n;
    if (mask && !mask[b]) return;
    mean[i] = plan_prior(pos, goal, rv, b * A, dt);
    std[i] = make_double2(init_std, init_std);
}

// The unicycle prior: lane = env, t sequential.  A lane stores n consecutive 16-byte rows of mean and of std.
__global__ __launch_bounds__(kPlanBlock) void plan_reset_uni_kernel(int B, int A, int n, double dt, double init_std, double std_rotation,
                                                                    double max_rotation, const double2* pos, const double2* goal,
                                                                    const double2* rv, const double* theta, const uint8_t* mask,
                                                                    double2* mean, double2* std) {
    const size_t b = (size_t)blockIdx.x * kPlanBlock + threadIdx.x;
    if (b >= (size_t)B) return;
    if (mask && !mask[b]) return;
    plan_prior_uni(pos, goal, rv, theta, b, A, n, dt, max_rotation, mean);
    for (int t = 0; t < n; ++t) std[b * n + t] = make_double2(init_std, std_rotation);
}

// Streaming: consecutive lanes write consecutive 16-byte rows (t fastest).  The counter words are (t, k, b, counter), so a row
// does not depend on B, K or n.
template <bool UNI>
__device__ __forceinline__ void plan_draw_lane(int B, int A, int K, int n, uint32_t seed_lo, uint32_t seed_hi, uint32_t counter,
                                               double max_rotation, const double2* rv, const double2* mean, const double2* std,
                                               double2* candidates) {
    const size_t i = (size_t)blockIdx.x * kPlanBlock + threadIdx.x;
    if (i >= (size_t)B * K * n) return;
    const uint32_t t = (uint32_t)(i % n), k = (uint32_t)((i / n) % K), b = (uint32_t)(i / ((size_t)n * K));
    const size_t row = (size_t)b * n + t;
    double2 a = mean[row];
    if (k > 0) {
        const PlanWords r4 = philox4x32_10(t, k, b, counter, seed_lo, seed_hi);
        const double u1 = ((double)(r4.w[0] >> 5) * 67108864.0 + (double)(r4.w[1] >> 6) + 1.0) / 9007199254740992.0;
        const double u2 = ((double)(r4.w[2] >> 5) * 67108864.0 + (double)(r4.w[3] >> 6)) / 9007199254740992.0;
        const double r = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
        const double2 sd = std[row];
        a.x = a.x + sd.x * (r * cos(ang));
        a.y = a.y + sd.y * (r * sin(ang));
    }
    candidates[i] = plan_clip<UNI>(a, rv[(size_t)b * A].y, max_rotation);
}
__global__ __launch_bounds__(kPlanBlock) void plan_draw_kernel(int B, int A, int K, int n, uint32_t seed_lo, uint32_t seed_hi,
                                                               uint32_t counter, const double2* rv, const double2* mean,
                                                               const double2* std, double2* candidates) {
    plan_draw_lane<false>(B, A, K, n, seed_lo, seed_hi, counter, 0.0, rv, mean, std, candidates);
}
// ... rows (v, r), clipped to the box
__global__ __launch_bounds__(kPlanBlock) void plan_draw_uni_kernel(int B, int A, int K, int n, uint32_t seed_lo, uint32_t seed_hi,
                                                                   uint32_t counter, double max_rotation, const double2* rv,
                                                                   const double2* mean, const double2* std, double2* candidates) {
    plan_draw_lane<true>(B, A, K, n, seed_lo, seed_hi, counter, max_rotation, rv, mean, std, candidates);
}

// rank(k) = #{j : s_j > s_k, or s_j == s_k and j < k} over the env's scores in LDS: a permutation of 0..K-1 for finite scores
// (NaN is not handled).  The one ranking rule of the refit and of the MPPI update.
__device__ inline int plan_rank(const double* sc, int K, int k) {
    const double sk = sc[k];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
        const double sj = sc[j];
        rank += (sj > sk || (sj == sk && j < k)) ? 1 : 0;
    }
    return rank;
}

// One wave per env.  LDS holds the env's scores and the elite indices, nothing else.
__global__ __launch_bounds__(64) void plan_refit_kernel(int K, int n, int E, int keep_best, double smoothing, double min_std,
                                                        const double* score, const double2* candidates, double* mean, double* std,
                                                        double2* best_actions, double* best_score, double2* action, int32_t* order) {
    __shared__ double sc[kPlanMaxCandidates];
    __shared__ int elite[kPlanMaxElites];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const double held = best_score[b];  // (read by every lane before lane 0 may replace it below)
    for (int k = lane; k < K; k += 64) sc[k] = score[b * K + k];
    elite[lane] = 0;  // (NaN scores rank nothing sensibly; the indices read below still address the env's own candidates)
    __syncthreads();
    for (int k = lane; k < K; k += 64) {
        const int rank = plan_rank(sc, K, k);
        if (order) order[b * K + rank] = k;
        if (rank < E) elite[rank] = k;
    }
    __syncthreads();
    const int top = elite[0];
    const double s_top = sc[top];
    if (!keep_best || s_top > held) {  // strict: the earliest holder of a score keeps it
        const double2* src = candidates + (b * K + top) * n;
        for (int t = lane; t < n; t += 64) best_actions[b * n + t] = src[t];
        if (lane == 0) {
            best_score[b] = s_top;
            action[b] = src[0];
        }
    }
    const double* cand = reinterpret_cast<const double*>(candidates);
    const double keep = 1.0 - smoothing;
    for (int c = lane; c < 2 * n; c += 64) {  // component (t, xy) of the plan: sums over the elites in rank order
        double sum = 0.0;
        for (int e = 0; e < E; ++e) sum = sum + cand[(b * K + elite[e]) * n * 2 + c];
        const double m = sum / (double)E;
        double dev2 = 0.0;
        for (int e = 0; e < E; ++e) {
            const double d = cand[(b * K + elite[e]) * n * 2 + c] - m;
            dev2 = dev2 + d * d;
        }
        const double sd = sqrt(dev2 / (double)E);
        const size_t at = b * n * 2 + c;
        mean[at] = smoothing * mean[at] + keep * m;
        const double blended = smoothing * std[at] + keep * sd;
        std[at] = blended < min_std ? min_std : blended;
    }
}

// One wave per env: the refit's ranks and best row, then every candidate weighted by exp((s_k - s_max) / temperature).  LDS holds
// the env's scores, its weights, the rank-0 index and the new first mean row (16 KiB + 24 bytes).  Lane = component (t, xy), the
// k loops sequential and the same in every lane: candidates[b] is streamed once for the mean and, with fit_std, once more for
// the deviation, consecutive lanes reading consecutive doubles of one row.  `action` is the updated mean's first row clipped
// as the draw clips, NOT the best row's.
__global__ __launch_bounds__(64) void plan_mppi_kernel(int A, int K, int n, int fit_std, int keep_best, double temperature,
                                                       double smoothing, double min_std, const double* score,
                                                       const double2* candidates, const double2* rv, double* mean, double* std,
                                                       double2* best_actions, double* best_score, double2* action, int32_t* order) {
    constexpr bool UNI = false;
    const double max_rotation = 0.0;
#include "plan_mppi_body.inc"
}
// ... the first row (v, r), clipped to the box
__global__ __launch_bounds__(64) void plan_mppi_uni_kernel(int A, int K, int n, int fit_std, int keep_best, double temperature,
                                                           double smoothing, double min_std, double max_rotation, const double* score,
                                                           const double2* candidates, const double2* rv, double* mean, double* std,
                                                           double2* best_actions, double* best_score, double2* action,
                                                           int32_t* order) {
    constexpr bool UNI = true;
#include "plan_mppi_body.inc"
}

// After a real step.  In place, so one lane owns component c of env b and walks t upwards (row t + 1 is read before it is
// written).  cur_steps == 0: the env's episode has just ended and its next scenario is loaded — or it is still waiting for one,
// and gets the prior of its stale state.
__global__ __launch_bounds__(kPlanBlock) void plan_shift_kernel(int B, int A, int n, double dt, double init_std, const double2* pos,
                                                                const double2* goal, const double2* rv, const uint8_t* active,
                                                                const int32_t* cur_steps, double* mean, double* std) {
    const int i = blockIdx.x * kPlanBlock + threadIdx.x;
    if (i >= 2 * B) return;
    const size_t b = (size_t)(i >> 1);
    const int c = i & 1;
    if (!active[b]) return;
    double* m = mean + b * n * 2 + c;
    double* s = std + b * n * 2 + c;
    if (cur_steps[b] == 0) {
        const double2 prior = plan_prior(pos, goal, rv, b * A, dt);
        const double v = c ? prior.y : prior.x;
        for (int t = 0; t < n; ++t) m[2 * t] = v;
    } else {
        for (int t = 0; t + 1 < n; ++t) m[2 * t] = m[2 * (t + 1)];
    }
    for (int t = 0; t < n; ++t) s[2 * t] = init_std;
}

// The unicycle form: the same lanes; the shifted envs walk t per component as above.  A re-seeded env's prior is a recurrence
// over both components, so its component-0 lane writes the whole 16-byte rows of the mean and its component-1 lane only its
// deviations (init_std for v, std_rotation for r).
__global__ __launch_bounds__(kPlanBlock) void plan_shift_uni_kernel(int B, int A, int n, double dt, double init_std, double std_rotation,
                                                                    double max_rotation, const double2* pos, const double2* goal,
                                                                    const double2* rv, const double* theta, const uint8_t* active,
                                                                    const int32_t* cur_steps, double* mean, double* std) {
    const int i = blockIdx.x * kPlanBlock + threadIdx.x;
    if (i >= 2 * B) return;
    const size_t b = (size_t)(i >> 1);
    const int c = i & 1;
    if (!active[b]) return;
    double* m = mean + b * n * 2 + c;
    double* s = std + b * n * 2 + c;
    if (cur_steps[b] == 0) {
        if (c == 0) plan_prior_uni(pos, goal, rv, theta, b, A, n, dt, max_rotation, reinterpret_cast<double2*>(mean));
    } else {
        for (int t = 0; t + 1 < n; ++t) m[2 * t] = m[2 * (t + 1)];
    }
    const double sd = c ? std_rotation : init_std;
    for (int t = 0; t < n; ++t) s[2 * t] = sd;
}

// The shipped predictors (cn_predict; crowdnav_amd/predict.py restates them on a host copy of the state bit for bit):
// human_vel[b][m][t][h] from the engine's state as it stands.  Lane = (env, mode, human), h fastest, so the lanes of one
// (env, mode) store consecutive 16-byte rows of step t; the lane reads its human once and walks t sequentially (to_goal is a
// recurrence in the position).  No LDS, no barrier, nothing of the engine written.  `models` holds the CN_PREDICT_* value of
// mode m in bits 4 m .. 4 m + 3: the M <= 8 models travel by value in one argument word, so no lane indexes an argument array.
constexpr int kPredictMaxModes = 8;
__host__ __device__ inline uint32_t predict_model_bits(int m, uint32_t model) { return model << (4 * m); }

__global__ __launch_bounds__(kPlanBlock) void predict_kernel(int B, int A, int M, int n, double dt, uint32_t models,
                                                             const double2* pos, const double2* vel, const double2* goal,
                                                             const double2* rv, double2* human_vel) {
    const size_t i = (size_t)blockIdx.x * kPlanBlock + threadIdx.x;
    const size_t H = (size_t)(A - 1);
    if (i >= (size_t)B * M * H) return;
    const size_t h = i % H, bm = i / H, b = bm / M;
    const uint32_t model = (models >> (4 * (uint32_t)(bm % M))) & 0xfu;
    const size_t agent = b * A + h + 1;
    double2* out = human_vel + bm * n * H + h;
    if (model == 0u) {  // CN_PREDICT_CONSTANT_VELOCITY: the velocity the human has, at every step
        const double2 v = vel[agent];
        for (int t = 0; t < n; ++t) out[(size_t)t * H] = v;
        return;
    }
    // CN_PREDICT_TO_GOAL, predict.to_goal line for line: straight for the goal at v_pref, the last step shortened to land on it
    double2 p = pos[agent];
    const double2 g = goal[agent];
    const double v_pref = rv[agent].y;
    const double reach = v_pref * dt;
    for (int t = 0; t < n; ++t) {
        const double dx = g.x - p.x, dy = g.y - p.y;
        const double dist = sqrt(dx * dx + dy * dy);
        double2 v = make_double2(0.0, 0.0);
        if (dist > 0.0) {
            if (dist <= reach) v = make_double2(dx / dt, dy / dt);
            else v = make_double2((dx / dist) * v_pref, (dy / dist) * v_pref);
        }
        out[(size_t)t * H] = v;
        p.x = p.x + v.x * dt;
        p.y = p.y + v.y * dt;
    }
}

// Hypotheses about where the humans are heading (cn_goal_hypotheses; crowdnav_amd/predict.py's goal_hypotheses restates it):
// goals[b][m][h] for cn_predict_orca_goals, from the engine's state as it stands.  Lane = (env, mode, human), h fastest: one
// 16-byte store per lane, consecutive lanes consecutive rows.  No LDS, nothing of the engine written.  The nominal offset d of
// a human is its goal's (heading = 0: g - p) or `reach` along its velocity (heading = 1; a standing human stays: d = 0); mode 0
// under nominal_first is p + d (the goal row itself, bit for bit, when heading = 0); every other mode turns d by
// std_heading z1 and stretches it by 1 + std_distance z2 (not below 0), (z1, z2) the Box-Muller pair of plan_draw_lane from one
// Philox block on the counter words (h, m, b, counter): a row depends on neither B, M nor H.  Every product, quotient and sum
// is an operation of its own in the order written.  A parked placeholder of the `mixed` rule is at rest at its goal, so
// d = 0 under either base and its row is its goal.
__global__ __launch_bounds__(kPlanBlock) void goal_hypotheses_kernel(int B, int A, int M, int heading, int nominal_first, double reach,
                                                                     double std_heading, double std_distance, uint32_t seed_lo,
                                                                     uint32_t seed_hi, uint32_t counter, const double2* pos,
                                                                     const double2* vel, const double2* goal, double2* goals) {
    const size_t i = (size_t)blockIdx.x * kPlanBlock + threadIdx.x;
    const size_t H = (size_t)(A - 1);
    if (i >= (size_t)B * M * H) return;
    const size_t h = i % H, bm = i / H, b = bm / M, m = bm % M;
    const size_t agent = b * A + h + 1;
    const double2 p = pos[agent], g = goal[agent];
    double dx = 0.0, dy = 0.0;
    if (heading) {
        const double2 v = vel[agent];
        const double speed = sqrt(v.x * v.x + v.y * v.y);
        if (speed > 0.0) dx = (v.x / speed) * reach, dy = (v.y / speed) * reach;
    } else {
        dx = g.x - p.x, dy = g.y - p.y;
    }
    if (m == 0 && nominal_first) {
        goals[i] = heading ? make_double2(p.x + dx, p.y + dy) : g;
        return;
    }
    const PlanWords r4 = philox4x32_10((uint32_t)h, (uint32_t)m, (uint32_t)b, counter, seed_lo, seed_hi);
    const double u1 = ((double)(r4.w[0] >> 5) * 67108864.0 + (double)(r4.w[1] >> 6) + 1.0) / 9007199254740992.0;
    const double u2 = ((double)(r4.w[2] >> 5) * 67108864.0 + (double)(r4.w[3] >> 6)) / 9007199254740992.0;
    const double r = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
    const double z1 = r * cos(ang), z2 = r * sin(ang);
    const double rot = std_heading * z1;
    double scale = 1.0 + std_distance * z2;
    if (scale < 0.0) scale = 0.0;
    const double c = cos(rot), s = sin(rot);
    goals[i] = make_double2(p.x + scale * (c * dx - s * dy), p.y + scale * (s * dx + c * dy));
}

}  // namespace cn
