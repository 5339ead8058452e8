// SARL robot decision on device — replaces, batched over B envs x K candidate actions,
//   MultiHumanRL.predict                     /root/reference crowd_nav/policy/multi_human_rl.py:11-63
//   CrowdSim.onestep_lookahead (reward part) crowd_sim/envs/crowd_sim.py:314-389 (via step_core-compatible code)
//   CADRL.propagate / rotate                 crowd_nav/policy/cadrl.py:104-129, 187-222
//   MultiHumanRL.build_occupancy_maps        multi_human_rl.py:109-163
//   sarl.ValueNetwork.forward                crowd_nav/policy/sarl.py:28-65 (mlp(): cadrl.py:11-19)
//
// Kernels (launched back to back on the engine's stream by cn_sarl_select):
//   orca_kernel            (step_kernels.h) the humans' next velocities — computed ONCE per env: they do not
//                          depend on the candidate action
//   sarl_lookahead_kernel  lane = (env, human): next human observable states (float64) and their occupancy maps — only with_om
//                          or under LSTM-RL's re-ordering; otherwise the feature kernel derives the next states itself
//   sarl_feature_kernel    lane = (env, action, human): float32 rotated 13-vector (+48 map values) -> X
//   the value network      on FP32 MFMA (v_mfma_f32_16x16x4_f32: exact f32, k-ordered fma chain): sarl_lds_kernels.h (workgroup =
//                          16 (env, action) groups x H humans, activations in LDS), sarl_narrow_kernel.h (a few decisions),
//                          sarl_reg_kernel.h (in registers).  Here: the kernels around it; sarl_net.h: its types and building blocks
//   sarl_select_kernel     wave = env: float64 reward of onestep_lookahead(action) (sarl_reward_of) + gamma^(dt v_pref) * V for
//                          every action, first strict maximum
//
// The tile row order, the fragment order of the activations and the network's building blocks: sarl_net.h.  This header's
// kernels are not templates: it belongs to one translation unit (sarl_abi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "orca_device.h"     // wave_lds_sync
#include "sarl_net.h"
#include "scenario_device.h"  // norm2
#include "transition.h"

namespace cn {

// torch.nn.Linear weight [N][K] (row-major) -> MFMA B fragments
__global__ void sarl_pack_kernel(const float* W, const float* bias, int N, int K, int k_offset, int k_count,
                                 int kpad, int ctiles, float* wp, float* bp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = ctiles * kpad * 64;
    if (idx < total) {
        const int lane = idx & 63;
        const int frag = idx >> 6;
        const int ct = frag / kpad, ks = frag - ct * kpad;
        const int n = ct * 16 + (lane & 15);
        const int k = ks * 4 + (lane >> 4);
        wp[idx] = (n < N && k < k_count) ? W[(size_t)n * K + k_offset + k] : 0.0f;
    }
    if (idx < ctiles * 16) bp[idx] = (bias && idx < N) ? bias[idx] : 0.0f;
}

// All layers of a network in ONE launch (cn_sarl_set_weights runs once per sampled episode in the RL phase: eleven launches of
// the kernel above were ~50 us of host and device time each time).  Block b belongs to the job whose block range holds it.
__global__ void sarl_pack_many_kernel(PackJobs jobs) {
    int j = 0;
    for (int i = 1; i < jobs.n; ++i) j = (int)blockIdx.x >= jobs.job[i].first_block ? i : j;
    const PackJob J = jobs.job[j];
    const int idx = ((int)blockIdx.x - J.first_block) * blockDim.x + threadIdx.x;
    const int total = J.ctiles * J.kpad * 64;
    if (idx < total) {
        const int lane = idx & 63;
        const int frag = idx >> 6;
        const int ct = frag / J.kpad, ks = frag - ct * J.kpad;
        const int n = ct * 16 + (lane & 15);
        const int k = ks * 4 + (lane >> 4);
        J.wp[idx] = (n < J.N && k < J.k_count) ? J.W[(size_t)n * J.K + J.k_offset + k] : 0.0f;
    }
    if (idx < J.ctiles * 16) J.bp[idx] = (J.bias && idx < J.N) ? J.bias[idx] : 0.0f;
}

// ------------------------------------------------------------------------------------ lookahead / reward
// Occupancy map human i sees among the H humans of one env (multi_human_rl.py:109-163; the robot is not in it).
// state_of(j, px, py, vx, vy) yields human j's state; m receives cells * channels float32 values.
// CAP = kSarlMaxHumans: the per-human slots are registers (loops fully unrolled); CAP = kSarlAnyHumans: any crowd the
// engine holds (<= 63 humans), slots in private memory, runtime trip counts.
constexpr int kSarlAnyHumans = 64;
template <int CAP, class StateOf>
__device__ __forceinline__ void occupancy_map_cap(const SarlCfg& C, int i, StateOf state_of, float* m) {
    const int cells = C.cell_num * C.cell_num;
    const int ch = C.om_channels;
    const int nh = CAP == kSarlMaxHumans ? kSarlMaxHumans : C.H;
    constexpr int kOmUnroll = CAP == kSarlMaxHumans ? kSarlMaxHumans : 1;
    double px, py, vx, vy;
    state_of(i, px, py, vx, vy);
    const double my_angle = atan2(vy, vx);
    // every other human's cell and rotated velocity once ...
    int cell_of[CAP];
    double rvx[CAP], rvy[CAP];
#pragma unroll kOmUnroll
    for (int j = 0; j < nh; ++j) {
        cell_of[j] = -1;
        rvx[j] = rvy[j] = 0.0;
        if (j >= C.H || j == i) continue;
        double qx, qy, wx, wy;
        state_of(j, qx, qy, wx, wy);
        const double ox = qx - px, oy = qy - py;
        const double rotation = atan2(oy, ox) - my_angle;
        const double dist = sqrt(ox * ox + oy * oy);
        const double rx = cos(rotation) * dist, ry = sin(rotation) * dist;
        const double xi = floor(rx / C.cell_size + C.cell_num / 2.0);
        const double yi = floor(ry / C.cell_size + C.cell_num / 2.0);
        if (xi < 0 || xi >= C.cell_num || yi < 0 || yi >= C.cell_num) continue;
        cell_of[j] = (int)(C.cell_num * yi + xi);
        const double vrot = atan2(wy, wx) - my_angle;
        const double speed = sqrt(wx * wx + wy * wy);
        rvx[j] = cos(vrot) * speed;
        rvy[j] = sin(vrot) * speed;
    }
    // ... then per cell: count, sum vx', sum vy' in visit order (python sum(): 0 + x1 + x2 ...)
    for (int cell = 0; cell < cells; ++cell) {
        double cnt = 0.0, svx = 0.0, svy = 0.0;
#pragma unroll kOmUnroll
        for (int j = 0; j < nh; ++j) {
            if (cell_of[j] != cell) continue;
            cnt += 1.0;
            svx += rvx[j];
            svy += rvy[j];
        }
        if (ch == 1) {
            m[cell] = cnt > 0.0 ? 1.0f : 0.0f;
        } else if (ch == 2) {
            m[2 * cell] = cnt > 0.0 ? (float)(svx / cnt) : 0.0f;
            m[2 * cell + 1] = cnt > 0.0 ? (float)(svy / cnt) : 0.0f;
        } else {
            m[3 * cell] = cnt > 0.0 ? (float)(cnt / cnt) : 0.0f;
            m[3 * cell + 1] = cnt > 0.0 ? (float)(svx / cnt) : 0.0f;
            m[3 * cell + 2] = cnt > 0.0 ? (float)(svy / cnt) : 0.0f;
        }
    }
}

template <class StateOf>
__device__ __forceinline__ void occupancy_map(const SarlCfg& C, int i, StateOf state_of, float* m) {
    if (C.H <= kSarlMaxHumans)
        occupancy_map_cap<kSarlMaxHumans>(C, i, state_of, m);
    else
        occupancy_map_cap<kSarlAnyHumans>(C, i, state_of, m);
}

// The same maps for the envs of ONE workgroup, spread over its lanes (sarl_decide_step_kernel: the maps of the next decision sit
// on a one-env sampling step's critical path, and a human's lane alone needs 1 + 4 x 2 float64 atan2 and 4 x 2 sincos in a
// row: +28 us).  The float64 operations of occupancy_map_cap, each exactly once and in the same expressions — only spread out:
//   phase 1  one item per human (its heading), per ordered pair (the other's bearing and distance) and per ordered pair again
//            (the other's velocity direction and speed): every atan2 / sqrt of the maps at once
//   phase 2  two items per ordered pair: cos / sin of the relative bearing -> cell; of the relative velocity direction -> (vx', vy')
//   phase 3  one item per (human, cell): count and velocity sums over the others IN INDEX ORDER (python's sum())
// so a map costs one atan2 and one sincos in a row.  state_of(e, j, px, py, vx, vy): human j of the workgroup's env e.
// scratch: (8 H + 52 H (H - 1)) bytes per env (H <= kSarlMaxHumans); sync(): the workgroup's barrier.
__host__ __device__ inline size_t occupancy_coop_bytes(int H) { return (size_t)8 * H + (size_t)52 * H * (H - 1); }
// map_of(e, i): where human i of env e's map (cells x channels floats) goes.
template <class StateOf, class Sync, class MapOf>
__device__ __forceinline__ void occupancy_maps_cooperative(const SarlCfg& C, int E, int tid, int threads, char* scratch, StateOf state_of,
                                                           Sync sync, MapOf map_of) {
    const int H = C.H, P = H * (H - 1);
    const size_t per_env = occupancy_coop_bytes(H);
    const auto ang_of = [&](int e) { return reinterpret_cast<double*>(scratch + e * per_env); };
    const auto pa_of = [&](int e) { return reinterpret_cast<double2*>(scratch + e * per_env + 8 * H); };           // (bearing, velocity direction)
    const auto pd_of = [&](int e) { return reinterpret_cast<double2*>(scratch + e * per_env + 8 * H + 16 * P); };  // (distance, speed)
    const auto pr_of = [&](int e) { return reinterpret_cast<double2*>(scratch + e * per_env + 8 * H + 32 * P); };  // (vx', vy')
    const auto pc_of = [&](int e) { return reinterpret_cast<int*>(scratch + e * per_env + 8 * H + 48 * P); };      // cell or -1
    const int n1 = H + 2 * P;
    for (int it = tid; it < E * n1; it += threads) {
        const int e = it / n1, k = it - e * n1;
        double px, py, vx, vy;
        if (k < H) {
            state_of(e, k, px, py, vx, vy);
            ang_of(e)[k] = atan2(vy, vx);
        } else {
            const int q = k - H, p = q < P ? q : q - P;
            const int i = p / (H - 1), jj = p - i * (H - 1), j = jj < i ? jj : jj + 1;
            double qx, qy, wx, wy;
            state_of(e, j, qx, qy, wx, wy);
            if (q < P) {
                state_of(e, i, px, py, vx, vy);
                const double ox = qx - px, oy = qy - py;
                pa_of(e)[p].x = atan2(oy, ox);
                pd_of(e)[p].x = sqrt(ox * ox + oy * oy);
            } else {
                pa_of(e)[p].y = atan2(wy, wx);
                pd_of(e)[p].y = sqrt(wx * wx + wy * wy);
            }
        }
    }
    sync();
    for (int it = tid; it < E * 2 * P; it += threads) {
        const int e = it / (2 * P), q = it - e * 2 * P, p = q < P ? q : q - P;
        const int i = p / (H - 1);
        const double my_angle = ang_of(e)[i];
        if (q < P) {
            const double rotation = pa_of(e)[p].x - my_angle, dist = pd_of(e)[p].x;
            const double rx = cos(rotation) * dist, ry = sin(rotation) * dist;
            const double xi = floor(rx / C.cell_size + C.cell_num / 2.0);
            const double yi = floor(ry / C.cell_size + C.cell_num / 2.0);
            pc_of(e)[p] = (xi < 0 || xi >= C.cell_num || yi < 0 || yi >= C.cell_num) ? -1 : (int)(C.cell_num * yi + xi);
        } else {
            const double vrot = pa_of(e)[p].y - my_angle, speed = pd_of(e)[p].y;
            pr_of(e)[p] = make_double2(cos(vrot) * speed, sin(vrot) * speed);
        }
    }
    sync();
    const int cells = C.cell_num * C.cell_num, ch = C.om_channels;
    for (int it = tid; it < E * H * cells; it += threads) {
        const int e = it / (H * cells), r = it - e * H * cells, i = r / cells, cell = r - i * cells;
        double cnt = 0.0, svx = 0.0, svy = 0.0;
        for (int jj = 0; jj < H - 1; ++jj) {  // the others in index order
            const int p = i * (H - 1) + jj;
            if (pc_of(e)[p] != cell) continue;
            const double2 rv = pr_of(e)[p];
            cnt += 1.0;
            svx += rv.x;
            svy += rv.y;
        }
        float* m = map_of(e, i);
        if (ch == 1) {
            m[cell] = cnt > 0.0 ? 1.0f : 0.0f;
        } else if (ch == 2) {
            m[2 * cell] = cnt > 0.0 ? (float)(svx / cnt) : 0.0f;
            m[2 * cell + 1] = cnt > 0.0 ? (float)(svy / cnt) : 0.0f;
        } else {
            m[3 * cell] = cnt > 0.0 ? (float)(cnt / cnt) : 0.0f;
            m[3 * cell + 1] = cnt > 0.0 ? (float)(svx / cnt) : 0.0f;
            m[3 * cell + 2] = cnt > 0.0 ? (float)(svy / cnt) : 0.0f;
        }
    }
}
__device__ __forceinline__ bool occupancy_coop_ok(const SarlCfg& C, size_t scratch_bytes, int envs) {
    return C.H >= 2 && C.H <= kSarlMaxHumans && (size_t)envs * occupancy_coop_bytes(C.H) <= scratch_bytes;
}

// LstmRL.predict re-orders the humans of the joint state by DEcreasing distance to the robot (lstm_rl.py:96-103; python's
// sorted(..., reverse=True) is stable: equal distances keep their original order).  Returns the human that sits at
// position p of the sorted joint state: the one whose stable rank equals p.  Distances are numpy's 2-vector norm of
// (human.position - robot.position).
// THE rule, stated once for every joint state whatever holds it (the engine's arrays, a caller's state8 rows): agent_pos(0) is
// the robot's position, agent_pos(1 + j) human j's.  human_order_key: what the humans are ranked by; human j comes before
// human k when its key is larger, or equal with j < k.
template <class AgentPos>
__device__ __forceinline__ double human_order_key(AgentPos agent_pos, int j, bool slot_in_use = true) {
    // a parked (absent) human sorts behind every present one (and so does a slot beyond the crowd, which is not read)
    const size_t a = (size_t)1 + j;
    return (slot_in_use && !is_parked(agent_pos(a))) ? norm2(agent_pos(a).x - agent_pos(0).x, agent_pos(a).y - agent_pos(0).y) : -1.0 - j;
}
template <class AgentPos>
__device__ __forceinline__ int human_at_sorted_position(AgentPos agent_pos, int H, int p) {
    double d[kSarlAnyHumans];
    for (int j = 0; j < H; ++j) d[j] = human_order_key(agent_pos, j);
    int who = p;
    for (int j = 0; j < H; ++j) {
        int rank = 0;
        for (int k = 0; k < H; ++k) rank += (d[k] > d[j] || (d[k] == d[j] && k < j)) ? 1 : 0;
        who = rank == p ? j : who;
    }
    return who;
}
// ... of up to kSarlMaxHumans humans as a permutation in registers: perm[p] = the human at position p (identity beyond H)
template <class AgentPos>
__device__ __forceinline__ void humans_sorted_permutation(AgentPos agent_pos, int H, int* perm /*[kSarlMaxHumans]*/) {
    double d[kSarlMaxHumans];
#pragma unroll
    for (int j = 0; j < kSarlMaxHumans; ++j) d[j] = human_order_key(agent_pos, j, j < H);
#pragma unroll
    for (int j = 0; j < kSarlMaxHumans; ++j) {
        int rank = 0;
#pragma unroll
        for (int k = 0; k < kSarlMaxHumans; ++k) rank += (k < H && (d[k] > d[j] || (d[k] == d[j] && k < j))) ? 1 : 0;
#pragma unroll
        for (int p = 0; p < kSarlMaxHumans; ++p) perm[p] = (j < H && rank == p) ? j : perm[p];
    }
}
// ... the human at position h of a joint state of H humans: the register permutation up to kSarlMaxHumans, ranked on demand above
template <class AgentPos>
__device__ __forceinline__ int human_of_sorted_state(AgentPos agent_pos, int H, int h) {
    if (H > kSarlMaxHumans) return human_at_sorted_position(agent_pos, H, h);
    int perm[kSarlMaxHumans];
#pragma unroll
    for (int p = 0; p < kSarlMaxHumans; ++p) perm[p] = p;
    humans_sorted_permutation(agent_pos, H, perm);
    int me = h;
#pragma unroll
    for (int p = 0; p < kSarlMaxHumans; ++p) me = (p == h) ? perm[p] : me;
    return me;
}
__device__ inline int human_by_decreasing_distance(const double2* pos, size_t g0, int H, int p) {
    return human_at_sorted_position([&](size_t a) { return pos[g0 + a]; }, H, p);
}

// Next observable state of every human (get_next_observable_state, agent.py:63-74) from the ORCA velocities,
// and (with_om) the occupancy map each human would see among those next states.
__global__ void sarl_lookahead_kernel(SarlCfg C, const double2* pos, const double2* vel, const double2* rv,
                                      const float* orca_vel, double* next_obs /*[B][H][5]*/,
                                      float* om /*[B][H][cells*ch]*/) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= C.B * C.H) return;
    const int b = idx / C.H, i = idx - b * C.H;
    const int A = C.H + 1;
    const size_t g0 = (size_t)b * A;
    // query_env = true: the env's lookahead (ORCA velocities, env order).  query_env = false (multi_human_rl.py:39-40):
    // propagate(human_state, ActionXY(human_state.vx, human_state.vy)) — each human keeps its observed velocity — over
    // state.human_states, which LstmRL.predict has sorted by decreasing distance.
    auto next_of = [&](int j, double& px, double& py, double& vx, double& vy) {
        const int src = C.sort_lookahead ? human_by_decreasing_distance(pos, g0, C.H, j) : j;
        const size_t gj = g0 + 1 + src;
        if (C.const_vel) {
            vx = vel[gj].x, vy = vel[gj].y;
        } else {
            vx = orca_vel[2 * gj], vy = orca_vel[2 * gj + 1];
        }
        px = pos[gj].x + vx * C.dt, py = pos[gj].y + vy * C.dt;
    };
    double px, py, vx, vy;
    next_of(i, px, py, vx, vy);
    const int me = C.sort_lookahead ? human_by_decreasing_distance(pos, g0, C.H, i) : i;
    double* o = next_obs + (size_t)idx * 5;
    o[0] = px, o[1] = py, o[2] = vx, o[3] = vy, o[4] = rv[g0 + 1 + me].x;
    if (C.with_om) occupancy_map(C, i, next_of, om + (size_t)idx * C.cell_num * C.cell_num * C.om_channels);
}

// Reward of onestep_lookahead(action) for every (env, action) (crowd_sim.py:331-389, update = False).
// (a device function: sarl_select_kernel evaluates it where it combines reward and value — one kernel and one stream boundary
// less per decision, which is 10 % of a single-env decision)
__device__ inline double sarl_reward_of(const SarlCfg& C, const double2* pos, const double2* vel, const double2* goal,
                                        const double2* rv, const double* gtime, const double* theta,
                                        const double* actions /*[K][2]*/, int b, int a) {
    const int A = C.H + 1;
    const size_t g0 = (size_t)b * A;
    double ax = actions[2 * a], ay = actions[2 * a + 1];
    const double rot_v = ax, rot_r = ay;
    if (C.unicycle) {
        ax = rot_v * cos(rot_r + theta[b]);
        ay = rot_v * sin(rot_r + theta[b]);
    }
    const double2 rp = pos[g0];
    const double rrad = rv[g0].x;
    double dmin = __builtin_inf();
    bool collision = false;
    if (C.const_vel) {
        // MultiHumanRL.compute_reward(next_self_state, next_human_states) (multi_human_rl.py:65-88): end-point distances
        // only, its own hard-coded constants (-0.25, 1, 0.2, 0.5), no time limit
        double nx = rp.x + ax * C.dt, ny = rp.y + ay * C.dt;
        if (C.unicycle) {
            const double th = theta[b] + rot_r;
            nx = rp.x + rot_v * cos(th) * C.dt;  // cadrl.py:120-124: next_vx = v cos(next_theta); px + next_vx * dt
            ny = rp.y + rot_v * sin(th) * C.dt;
        }
        for (int i = 1; i < A; ++i) {
            const double2 hp = pos[g0 + i], hv = vel[g0 + i];
            const double hx = hp.x + hv.x * C.dt, hy = hp.y + hv.y * C.dt;
            const double dist = norm2(nx - hx, ny - hy) - rrad - rv[g0 + i].x;
            if (dist < 0.0) {
                collision = true;
                break;
            }
            if (dist < dmin) dmin = dist;
        }
        const double2 gl = goal[g0];
        const bool reaching = norm2(nx - gl.x, ny - gl.y) < rrad;
        double r;
        if (collision) {
            r = -0.25;
        } else if (reaching) {
            r = 1.0;
        } else if (dmin < 0.2) {
            r = (dmin - 0.2) * 0.5 * C.dt;
        } else {
            r = 0.0;
        }
        return r;
    }
    for (int i = 1; i < A; ++i) {
        const double2 hp = pos[g0 + i], hv = vel[g0 + i];
        const double2 cp = closest_point(hp.x - rp.x, hp.y - rp.y, hv.x - ax, hv.y - ay, C.dt);  // (transition.h)
        const double d = norm2(cp.x, cp.y);
        const double c = d - rv[g0 + i].x - rrad;
        if (c < 0.0) {
            collision = true;
            break;
        } else if (c < dmin) {
            dmin = c;
        }
    }
    double endx = rp.x + ax * C.dt, endy = rp.y + ay * C.dt;
    if (C.unicycle) {
        const double th = theta[b] + rot_r;
        endx = rp.x + cos(th) * rot_v * C.dt;
        endy = rp.y + sin(th) * rot_v * C.dt;
    }
    const double2 gl = goal[g0];
    const bool reaching = norm2(endx - gl.x, endy - gl.y) < rrad;
    double r;
    if (gtime[b] >= C.time_limit - 1.0) {
        r = 0.0;
    } else if (collision) {
        r = C.collision_penalty;
    } else if (reaching) {
        r = C.success_reward;
    } else if (dmin < C.discomfort_dist) {
        r = (dmin - C.discomfort_dist) * C.discomfort_factor * C.dt;
    } else {
        r = 0.0;
    }
    return r;
}

// ------------------------------------------------------------------------------------ features
// CADRL.rotate (cadrl.py:187-222) of one float32 joint row [self (9) | human (5)]: one rounding per torch op.
__device__ __forceinline__ void rotate_row(float px, float py, float vx, float vy, float radius, float gx, float gy,
                                           float v_pref, float theta, int unicycle, float px1, float py1, float vx1,
                                           float vy1, float radius1, float* f) {
    const float dx = gx - px, dy = gy - py;
    const float rot = atan2f(dy, dx);
    const float dg = sqrtf(dx * dx + dy * dy);
    const float c = cosf(rot), s = sinf(rot);
    f[0] = dg;
    f[1] = v_pref;
    f[2] = unicycle ? theta - rot : 0.0f;  // cadrl.py:207-211
    f[3] = radius;
    f[4] = vx * c + vy * s;
    f[5] = vy * c - vx * s;
    f[6] = (px1 - px) * c + (py1 - py) * s;
    f[7] = (py1 - py) * c - (px1 - px) * s;
    f[8] = vx1 * c + vy1 * s;
    f[9] = vy1 * c - vx1 * s;
    f[10] = radius1;
    const float ex = px - px1, ey = py - py1;
    f[11] = sqrtf(ex * ex + ey * ey);
    f[12] = radius + radius1;
}

// The occupancy-map columns of X (features 13.. and the zero padding) for every (group, human) row: what
// sarl_feature_kernel leaves out with om_cols = 0.  Only cn_sarl_export uses it, so that an exported X is the whole input
// matrix of the value network whichever way the kernel read it.
__global__ void sarl_om_columns_kernel(SarlCfg C, int in_dim, int ks_x, const float* om, float* X, size_t n_tiles) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_tiles * C.H * kSarlGroups) return;
    const int g = (int)(idx % kSarlGroups);
    const int h = (int)((idx / kSarlGroups) % C.H);
    const size_t tile = idx / ((size_t)kSarlGroups * C.H);
    const size_t G = tile * kSarlGroups + g;
    if (G >= (size_t)C.B * C.n_actions) return;  // padding groups are zero already
    float* x = X + ((tile * C.H + h) * ks_x) * 64 + g;
    const int extra = in_dim - 13;
    const float* m = om + ((G / C.n_actions) * C.H + h) * (size_t)extra;
    for (int k = 0; k < extra; ++k) x[((13 + k) >> 2) * 64 + ((13 + k) & 3) * 16] = m[k];  // (tile_word(13 + k), spelled out: the call moves this kernel's assembly)
    for (int n = in_dim; n < ks_x * 4; ++n) x[tile_word(n)] = 0.0f;
}

// The 13 rotated features of X row (env b, action a, human h): CADRL.rotate of the float32 joint row
// [propagate(self, action) (9) | next human state (5)] — shared by sarl_feature_kernel (X in HBM) and sarl_narrow_kernel (X
// built in LDS by the kernel that consumes it).
__device__ __forceinline__ void sarl_feature_row(const SarlCfg& C, int b, int a, int h, const double2* pos, const double2* goal,
                                                 const double2* rv, const double* theta, const double* actions,
                                                 double* next_obs, const double2* vel, const float* orca_vel, float* f) {
    const size_t g0 = (size_t)b * (C.H + 1);
    // propagate(self_state, action) in float64 (cadrl.py:113-118), then torch.Tensor([...]) narrows to float32
    double ax = actions[2 * a], ay = actions[2 * a + 1];
    float theta_f = 0.0f;
    if (C.unicycle) {  // cadrl.py:119-125: next_theta = theta + r, velocity v (cos, sin)(next_theta)
        const double th = theta[b] + ay, v = ax;
        ax = v * cos(th);
        ay = v * sin(th);
        theta_f = (float)th;
    }
    const float px = (float)(pos[g0].x + ax * C.dt), py = (float)(pos[g0].y + ay * C.dt);
    const float vx = (float)ax, vy = (float)ay;
    const float radius = (float)rv[g0].x, v_pref = (float)rv[g0].y;
    const float gx = (float)goal[g0].x, gy = (float)goal[g0].y;
    // the human's next observable state (get_next_observable_state, agent.py:63-74): from sarl_lookahead_kernel when it ran
    // (occupancy maps, LSTM-RL's re-ordering); otherwise computed here — the same float64 expressions — and written out by the
    // lanes of the env's first action (cn_sarl_export, the step's observation)
    double o[5];
    if (orca_vel != nullptr) {
        const size_t gj = g0 + 1 + h;
        const double vxn = C.const_vel ? vel[gj].x : (double)orca_vel[2 * gj], vyn = C.const_vel ? vel[gj].y : (double)orca_vel[2 * gj + 1];
        o[0] = pos[gj].x + vxn * C.dt, o[1] = pos[gj].y + vyn * C.dt, o[2] = vxn, o[3] = vyn, o[4] = rv[gj].x;
        if (a == 0) {
            double* dst = next_obs + ((size_t)b * C.H + h) * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) dst[k] = o[k];
        }
    } else {
        const double* src = next_obs + ((size_t)b * C.H + h) * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) o[k] = src[k];
    }
    const float px1 = (float)o[0], py1 = (float)o[1], vx1 = (float)o[2], vy1 = (float)o[3], radius1 = (float)o[4];
    rotate_row(px, py, vx, vy, radius, gx, gy, v_pref, theta_f, C.unicycle, px1, py1, vx1, vy1, radius1, f);
}

// X row of (env b, action a, human h): CADRL.rotate of the float32 joint row
// [propagate(self, action) (9) | next human state (5)] (+ the human's occupancy map), written straight in the MLP
// kernel's LDS order: group G = b * K + a -> tile G / 16, g = G % 16, row tile = h;
// X[((tile * H + h) * ks_x + n / 4) * 64 + (n % 4) * 16 + g] = feature n.  Lanes run over g fastest, so every
// store instruction writes 16 consecutive words per (tile, h).
__global__ void sarl_feature_kernel(SarlCfg C, int in_dim, int ks_x, const double2* pos, const double2* goal,
                                    const double2* rv, const double* theta, const double* actions,
                                    double* next_obs, const float* om, float* X, size_t n_tiles,
                                    int* hcount /*[n_tiles * 16] humans present per group*/,
                                    int om_cols = 1 /* 0: the consumer reads the occupancy maps from `om` itself (they do
                                    not depend on the action: written into X they are 81 copies, 48 of every 61 floats);
                                    only k-steps 0..3 — the 13 rotated features and map values 0..2 — are written */,
                                    const double2* vel = nullptr, const float* orca_vel = nullptr /* not null: no lookahead kernel ran */) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_tiles * C.H * kSarlGroups) return;
    const int g = (int)(idx % kSarlGroups);
    const int h = (int)((idx / kSarlGroups) % C.H);
    const size_t tile = idx / ((size_t)kSarlGroups * C.H);
    const size_t G = tile * kSarlGroups + g;
    float* x = X + ((tile * C.H + h) * ks_x) * 64 + g;
    if (G >= (size_t)C.B * C.n_actions) {  // padding groups of the last tile: finite zeros
        for (int n = 0; n < ks_x * 4; ++n) x[tile_word(n)] = 0.0f;
        if (h == 0) hcount[tile * kSarlGroups + g] = C.H;
        return;
    }
    if (h == 0) {  // len(state.human_states): under the `mixed` rule the env's absent humans are parked behind the present ones
        const size_t e0 = (G / C.n_actions) * (size_t)(C.H + 1);
        int present = 0;
        for (int j = 0; j < C.H; ++j) present += is_parked(pos[e0 + 1 + j]) ? 0 : 1;
        hcount[tile * kSarlGroups + g] = present;
    }
    const int a = (int)(G % C.n_actions);
    const int b = (int)(G / C.n_actions);
    float f[13];
    sarl_feature_row(C, b, a, h, pos, goal, rv, theta, actions, next_obs, vel, orca_vel, f);
#pragma unroll
    for (int k = 0; k < 13; ++k) x[tile_word(k)] = f[k];
    const int extra = in_dim - 13;
    const float* m = om + ((size_t)b * C.H + h) * (extra > 0 ? extra : 0);
    const int n_om = om_cols ? extra : (extra < 3 ? extra : 3);
    for (int k = 0; k < n_om; ++k) x[((13 + k) >> 2) * 64 + ((13 + k) & 3) * 16] = m[k];  // (tile_word(13 + k), spelled out: the call moves this kernel's assembly)
    // (features in_dim .. 4 ks_x - 1 are never written by anyone: X is zero from its allocation — 7 of 20 floats per row at 13
    // inputs, and the kernel is bound by its HBM writes)
}

// ------------------------------------------------------------------------------------ replay-memory side
// MultiHumanRL.transform (multi_human_rl.py:90-104; CADRL.transform cadrl.py:171-185 when H = 1) of the CURRENT joint
// state of every env: rotate(float32 [self_state (9) | human h (5)]) (+ human h's occupancy map among the current
// human states) -> out[b][h][0..in_dim): the state a train-phase predict() leaves in policy.last_state and
// Explorer.update_memory pushes into the replay memory.  lane = (env, position in the joint state).
__device__ __forceinline__ void sarl_transform_row(const SarlCfg& C, int in_dim, int sort_humans, const double2* pos,
                                                   const double2* vel, const double2* goal, const double2* rv,
                                                   const double* theta, float* out, int64_t env_stride, int b, int h,
                                                   bool maps = true) {
    const size_t g0 = (size_t)b * (C.H + 1);
    // perm[p] = human at position p of the joint state.  LSTM-RL (sort_humans): LstmRL.predict re-orders the humans by
    // DEcreasing distance to the robot before MultiHumanRL.predict runs (lstm_rl.py:96-103; python's sorted(...,
    // reverse=True) is stable: equal distances keep their original order), so that is the order of last_state.
    int perm[kSarlMaxHumans];
#pragma unroll
    for (int p = 0; p < kSarlMaxHumans; ++p) perm[p] = p;
    if (sort_humans && C.H <= kSarlMaxHumans) humans_sorted_permutation([&](size_t a) { return pos[g0 + a]; }, C.H, perm);
    const bool big = C.H > kSarlMaxHumans;  // the register permutation holds kSarlMaxHumans; larger crowds rank on demand
    int me = h;  // env order unless sorted
    if (sort_humans && !big) {
#pragma unroll
        for (int p = 0; p < kSarlMaxHumans; ++p) me = (p == h) ? perm[p] : me;
    } else if (sort_humans) {
        me = human_by_decreasing_distance(pos, g0, C.H, h);
    }
    const size_t g1 = g0 + 1 + me;
    float f[13];
    rotate_row((float)pos[g0].x, (float)pos[g0].y, (float)vel[g0].x, (float)vel[g0].y, (float)rv[g0].x,
               (float)goal[g0].x, (float)goal[g0].y, (float)rv[g0].y, (float)theta[b], C.unicycle, (float)pos[g1].x,
               (float)pos[g1].y, (float)vel[g1].x, (float)vel[g1].y, (float)rv[g1].x, f);
    float* x = out + (size_t)b * env_stride + (size_t)h * in_dim;
#pragma unroll
    for (int k = 0; k < 13; ++k) x[k] = f[k];
    if (C.with_om && maps) {  // (maps = false: the caller's lanes share them, occupancy_maps_cooperative)
        auto state_of = [&](int j, double& px, double& py, double& vx, double& vy) {
            int oj = j;
            if (!big) {
#pragma unroll
                for (int p = 0; p < kSarlMaxHumans; ++p) oj = (p == j) ? perm[p] : oj;
            } else if (sort_humans) {
                oj = human_by_decreasing_distance(pos, g0, C.H, j);
            }
            const size_t gj = g0 + 1 + oj;
            px = pos[gj].x, py = pos[gj].y, vx = vel[gj].x, vy = vel[gj].y;
        };
        occupancy_map(C, h, state_of, x + 13);
    }
}
__global__ void sarl_transform_kernel(SarlCfg C, int in_dim, int sort_humans, const double2* pos, const double2* vel,
                                      const double2* goal, const double2* rv, const double* theta,
                                      float* out /*[B][H][in_dim]*/, int64_t env_stride /*floats between envs*/) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= C.B * C.H) return;
    const int b = idx / C.H;
    sarl_transform_row(C, in_dim, sort_humans, pos, vel, goal, rv, theta, out, env_stride, b, idx - b * C.H);
}

// cn_sarl_state_values: the same transform of joint states the CALLER holds in the env layout — state8 double [n][A][8] = px,
// py, vx, vy, gx, gy, radius, v_pref per agent (cn_get_state's rows; agent 0 the robot), theta double [n] or nullptr (0) — for
// states first .. first + count - 1 as the network input of one pass: state first + G is group G of the pass.  Narrowed to
// float32 where sarl_transform_row narrows, rotated by the same rotate_row, ordered by the same rule.  One lane per (group,
// human), indexed like sarl_feature_kernel's.  rows == nullptr: X in the MLP tile order, every word of a row written (features
// 13 .. 4 ks_x - 1 zero), padding groups of the last tile finite zeros, hcount = H throughout (no mixed rule here);
// otherwise rows [count][H][13] for the narrow kernel's caller-rows mode (SarlDecide::x_rows).
__global__ void sarl_state_feature_kernel(int H, int unicycle, int sort_humans, const double* state8, const double* theta,
                                          size_t first, size_t count, size_t n_tiles, int ks_x, float* X, int* hcount, float* rows) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_tiles * H * kSarlGroups) return;
    const int g = (int)(idx % kSarlGroups);
    const int h = (int)((idx / kSarlGroups) % H);
    const size_t tile = idx / ((size_t)kSarlGroups * H);
    const size_t G = tile * kSarlGroups + g;
    float* x = X + ((tile * H + h) * ks_x) * 64 + g;
    if (G >= count) {
        if (rows != nullptr) return;
        for (int n = 0; n < ks_x * 4; ++n) x[tile_word(n)] = 0.0f;
        if (h == 0) hcount[tile * kSarlGroups + g] = H;
        return;
    }
    // an agent's row is four double2: (px, py) (vx, vy) (gx, gy) (radius, v_pref)
    const double2* agents = reinterpret_cast<const double2*>(state8) + (first + G) * (size_t)(H + 1) * 4;
    const int me = sort_humans ? human_of_sorted_state([&](size_t a) { return agents[4 * a]; }, H, h) : h;
    const double2* other = agents + 4 * (size_t)(1 + me);
    const double2 p0 = agents[0], v0 = agents[1], g0 = agents[2], r0 = agents[3];
    const double2 p1 = other[0], v1 = other[1], r1 = other[3];
    const float th = theta != nullptr ? (float)theta[first + G] : 0.0f;
    float f[13];
    rotate_row((float)p0.x, (float)p0.y, (float)v0.x, (float)v0.y, (float)r0.x, (float)g0.x, (float)g0.y, (float)r0.y, th, unicycle,
               (float)p1.x, (float)p1.y, (float)v1.x, (float)v1.y, (float)r1.x, f);
    if (rows != nullptr) {
        float* r = rows + (G * H + h) * 13;
#pragma unroll
        for (int k = 0; k < 13; ++k) r[k] = f[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < 13; ++k) x[tile_word(k)] = f[k];
    for (int n = 13; n < ks_x * 4; ++n) x[tile_word(n)] = 0.0f;
    if (h == 0) hcount[tile * kSarlGroups + g] = H;
}

// cn_lookahead_values: the n-step return of every branch, score = ret + table[steps] * V(final state); a branch that ended
// (ReachGoal / Collision / Timeout) gets no bootstrap, as the TD target of an episode's last transition is the reward alone
// (explorer.py:107-113).  One multiply and one add, in that order (the build has -ffp-contract=off).  One lane per branch.
__global__ void lookahead_score_kernel(size_t n, const double* ret, const uint8_t* info, const int32_t* steps, const float* value,
                                       const double* table, int len, double* score) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double boot = 0.0;
    if (info[i] < CN_REACH_GOAL) {
        int t = steps[i];
        t = t < len - 1 ? t : len - 1;
        t = t < 0 ? 0 : t;
        boot = table[t] * (double)value[i];
    }
    score[i] = ret[i] + boot;
}

// The epsilon-greedy branch of MultiHumanRL.predict (multi_human_rl.py:28-31), on each env's OWN numpy stream — the
// one cn_reset seeded (np.random.seed in CrowdSim.reset, crowd_sim.py:272-276), continued after the scenario draws:
//   probability = np.random.random();  if probability < epsilon: action_space[np.random.choice(K)]
// np.random.choice(K) of the legacy RandomState is randint(0, K): 32-bit draws masked to the next power of two minus
// one, rejected while > K - 1.  An env already at its goal (best == -1) returned before the draw (:22-23).
// lane = env.  explored (optional) receives 1 where the random action replaced the greedy one.
// the draw itself: returns the random action's index, or -1 when the greedy action stands (or the env has no stream)
__device__ __forceinline__ int sarl_explore_draw(int B, int K, double epsilon, uint32_t* mt_key, int* mt_pos, int* error, int b) {
    if (mt_pos[b] < 0) {  // the env was not (re)started by cn_reset: there is no stream to continue
        atomicOr(error, 2);
        return -1;
    }
    Mt19937 rng{mt_key + b, B, mt_pos[b]};
    const double probability = rng.random();
    int picked = -1;
    if (probability < epsilon) {
        uint32_t bits = (uint32_t)(K - 1);
        bits |= bits >> 1, bits |= bits >> 2, bits |= bits >> 4, bits |= bits >> 8, bits |= bits >> 16;
        uint32_t k = 0;
        if (K > 1) do k = rng.next32() & bits; while (k > (uint32_t)(K - 1));  // randint(0, 1) draws nothing
        picked = (int)k;
    }
    mt_pos[b] = rng.pos;
    return picked;
}
__device__ __forceinline__ void sarl_explore_env(int B, int K, double epsilon, uint32_t* mt_key, int* mt_pos,
                                                 const double* actions, bool masked_out, int32_t* best, double* action,
                                                 uint8_t* explored, int* error, int b) {
    if (explored) explored[b] = 0;
    if (masked_out) return;
    if (best[b] == -1) return;
    const int k = sarl_explore_draw(B, K, epsilon, mt_key, mt_pos, error, b);
    if (k >= 0) {
        best[b] = (int32_t)k;
        action[2 * b] = actions[2 * k];
        action[2 * b + 1] = actions[2 * k + 1];
        if (explored) explored[b] = 1;
    }
}
__global__ void sarl_explore_kernel(int B, int K, double epsilon, uint32_t* mt_key, int* mt_pos, const double* actions,
                                    const uint8_t* mask, int32_t* best, double* action, uint8_t* explored,
                                    int* error) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    sarl_explore_env(B, K, epsilon, mt_key, mt_pos, actions, mask && !mask[b], best, action, explored, error, b);
}

// ------------------------------------------------------------------------------------ action selection
// value = reward + pow(gamma, time_step * v_pref) * V (multi_human_rl.py:52); the first strict maximum wins (:54);
// a robot already at its goal stops (:22-23, policy.py:43-49).  best = -1 encodes that stop action.
// The arg-max of env b -> best / action_out (one lane)
__device__ __forceinline__ void sarl_pick_tail(const SarlCfg& C, const double2* pos, const double2* goal, const double2* rv,
                                               const double* actions, int* best, double* action_out, int b, int bi) {
    const size_t g0 = (size_t)b * (C.H + 1);
    int arg = bi;
    const double dy = pos[g0].y - goal[g0].y, dx = pos[g0].x - goal[g0].x;
    const bool arrived = norm2(dy, dx) < rv[g0].x;  // np.linalg.norm((py - gy, px - gx))
    if (arrived) arg = -1;
    best[b] = (arrived || arg < 0) ? (arrived ? -1 : -2) : arg;  // -2: every value was NaN / -inf (:57-58)
    action_out[2 * b] = arg >= 0 ? actions[2 * arg] : 0.0;
    action_out[2 * b + 1] = arg >= 0 ? actions[2 * arg + 1] : 0.0;
}
// The wave's best (value, action) -> best / action_out of env b: a butterfly keeps the largest value, lowest index on ties
// (= the first strict maximum of the reference's loop; NaN and -inf never win: `value > max_value` is false)
__device__ __forceinline__ void sarl_pick_env(const SarlCfg& C, const double2* pos, const double2* goal, const double2* rv,
                                              const double* actions, int* best, double* action_out, int b, int lane, double bv,
                                              int bi) {
#pragma unroll
    for (int off = kWaveSize / 2; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        const bool take = oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi));
        bv = take ? ov : bv;
        bi = take ? oi : bi;
    }
    if (lane != 0) return;
    sarl_pick_tail(C, pos, goal, rv, actions, best, action_out, b, bi);
}
__device__ __forceinline__ void sarl_select_env(const SarlCfg& C, const double2* pos, const double2* vel, const double2* goal,
                                                const double2* rv, const double* gtime, const double* theta,
                                                const double* actions, double* reward, const float* V, double* values,
                                                int* best, double* action_out, int b, int lane) {
    // one wave per env: lanes stride over the actions
    double bv = -__builtin_inf();
    int bi = -1;
    for (int a = lane; a < C.n_actions; a += kWaveSize) {
        const double r = sarl_reward_of(C, pos, vel, goal, rv, gtime, theta, actions, b, a);  // onestep_lookahead's reward
        reward[(size_t)b * C.n_actions + a] = r;                                              // (kept for cn_sarl_export)
        const double v = r + C.gamma_bar * (double)V[(size_t)b * C.n_actions + a];
        if (values) values[(size_t)b * C.n_actions + a] = v;
        if (v > bv) {
            bv = v;
            bi = a;
        }
    }
    sarl_pick_env(C, pos, goal, rv, actions, best, action_out, b, lane, bv, bi);
}
__global__ void sarl_select_kernel(SarlCfg C, const double2* pos, const double2* vel, const double2* goal, const double2* rv,
                                   const double* gtime, const double* theta, const double* actions, double* reward,
                                   const float* V, double* values, int* best, double* action_out) {
    const int b = blockIdx.x * (blockDim.x / kWaveSize) + (threadIdx.x / kWaveSize);
    if (b >= C.B) return;
    sarl_select_env(C, pos, vel, goal, rv, gtime, theta, actions, reward, V, values, best, action_out, b,
                    threadIdx.x & (kWaveSize - 1));
}

// cn_sarl_sample_step outside the narrow route: the previous step's episode ends leave the set of sampling envs
__global__ void sarl_alive_kernel(int B, uint8_t* alive, const uint8_t* done) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && done[b]) alive[b] = 0;
}

// What cn_sarl_sample_step adds to the network kernel: value != nullptr -> every tile adds the lookahead reward of its groups and
// stores reward + gamma V, tile b writes env b's replay state; counter != nullptr -> the last workgroup decides as well (otherwise
// sarl_decide_step_kernel does, in front of the transition).
struct SarlDecide {
    int* counter;        // workgroups that have written their V (zero between launches)
    double epsilon;
    uint8_t* alive;      // [B] in/out
    const uint8_t* done; // [B] the previous step's episode-end flags
    int32_t* best;       // [B]
    double* action;      // [B][2]
    float* state_out;    // [B][H][in_dim] at env_stride floats between envs (may be null)
    int64_t env_stride;
    int sort_humans, in_dim;
    double* reward;      // [B][K]
    double* value;       // [B][K] reward + gamma^(dt v_pref) V, written by the tile that computed V
    const double* gtime; // [B]
    uint32_t* mt_key;
    int* mt_pos;
    int* error;
    // occupancy maps (round 6): what sarl_lookahead_kernel computes per (env, human) for the NEXT decision, written by
    // sarl_decide_step_kernel behind its ORCA pass (null without maps)
    double* next_obs_out;  // [B][H][5]
    float* om_out;         // [B][H][cells * channels]
    int side_wg;           // sarl_narrow_kernel: the LAST workgroup of the grid is not a tile — it writes the replay-memory states
    // cn_sarl_values (ABI v11): the rows come from the caller — joint states [ext_groups][H][13] float32 as cn_sarl_transform /
    // cn_sarl_sample_step wrote them (a replay memory's states) — instead of being built from the envs: V of each, nothing else
    const float* x_rows;
    int ext_groups;
};

}  // namespace cn
