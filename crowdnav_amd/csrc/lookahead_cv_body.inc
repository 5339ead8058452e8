// The lane body of lookahead_cv_kernel and lookahead_paths_kernel (lookahead_cv_kernel.h): the loads, the barrier and the book
// around the transition, whose arithmetic is transition.h's.  Included text, not a __device__ function, for rollout_body.inc's
// reason: as a __forceinline__ function taking the parameter block by reference or by value hipcc gave both instantiations of
// lookahead_cv_kernel another instruction stream (profiles/lookahead_paths_kernels.txt).  In scope where it is included: UNI,
// PATHS, GOAL (constexpr bool), P (CvParams), action_table, human_vel (nullptr without PATHS), goal_weight (0.0 without GOAL), Od.
// PATHS = false: the velocity a human chooses is the one it has.  PATHS = true: the velocity human h chooses at step t is
// human_vel[b][t][h] (include/crowdnav_amd.h, "Lookahead under predicted human motion") — step_core's transition with the
// humans' policy replaced by the table: the swept test of step t reads the velocity the human HAS when the step starts (its
// state velocity at t = 0, then the one it chose at step t - 1), the move and the state after the step take the chosen one.
//
// PATHS: h_vel is double-buffered exactly as h_pos is — the velocity a human has before step t in [t & 1], after it in
// [(t + 1) & 1].  Owner lane h < H loads row [b][t][h] at the top of iteration t (one 16-byte load, consecutive lanes
// consecutive rows; its latency hides behind the scan, which does not need it), moves its human with it, and before the barrier
// of iteration t publishes the position after step t in h_pos[(t + 1) & 1] and the velocity after step t in
// h_vel[(t + 1) & 1].  Only rows of steps the wave makes are loaded.  The race argument is the positions', for both arrays: the
// scan of iteration t reads [t & 1], published before the barrier of iteration t - 1 (or the first __syncthreads) and next
// written in iteration t + 1, behind the barrier of iteration t that every scanning lane has passed.  A lane whose branch ends
// at step t writes its final_state8 rows after the barrier of iteration t from [(t + 1) & 1] of both arrays — the position
// after its last step and the velocity of that step; those buffers are written again only in iteration t + 2, behind the
// barrier of iteration t + 1, which the ending lane reaches after its stores.  One barrier per step; the argument does not lean
// on the workgroup being a single wave.
//
// GOAL = true (include/crowdnav_amd.h, "Lookahead goal-progress term"): the lane keeps d0, the robot's distance to its goal as
// the engine holds it, from where the robot row is loaded, and stores ret + goal_weight * (d0 - d1) with d1 the distance
// after the branch's last transition — the position final_state8 reports.  One subtraction, one multiply, one add, after the
// last reward.  GOAL = false compiles to the instructions the kernels had (profiles/lookahead_goal_kernels.txt).
    __shared__ double2 h_pos[2][kCvHumans];  // position before the step in [t & 1], after it in [(t + 1) & 1]
    __shared__ double2 h_vel[PATHS ? 2 : 1][kCvHumans], h_goal[kCvHumans], h_rv[kCvHumans];
    const int lane = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)P.chunks), chunk = (int)(blockIdx.x - (unsigned)b * (unsigned)P.chunks);
    const int k = chunk * kWave + lane;
    const int H = P.A - 1;
    const size_t g0 = (size_t)b * (size_t)P.A;  // the env's robot row

    // PATHS: the env's velocity rows [n_steps][H] (a lane >= H forms no address from it)
    const double2* const vel_rows = reinterpret_cast<const double2*>(human_vel) + (size_t)b * (size_t)P.n_steps * (size_t)H;
    // this lane's human (lane h < H owns human slot h + 1): in registers for the whole launch
    double hx = 0.0, hy = 0.0, hvx = 0.0, hvy = 0.0;
    if (lane < H) {
        const double2 p = P.pos[g0 + 1 + lane], v = P.vel[g0 + 1 + lane];
        hx = p.x, hy = p.y, hvx = v.x, hvy = v.y;
        h_pos[0][lane] = p, h_vel[0][lane] = v;
        h_goal[lane] = P.goal[g0 + 1 + lane], h_rv[lane] = P.rv[g0 + 1 + lane];
    }
    // this lane's branch: the robot as env b holds it, a fresh book
    bool running = k < P.K;
    const size_t v_env = (size_t)b * (size_t)P.K + (size_t)(running ? k : 0);  // (a tail lane forms no address of its own)
    double px = 0.0, py = 0.0, vx = 0.0, vy = 0.0, gx = 0.0, gy = 0.0, rad = 0.0, vpref = 0.0, theta = 0.0, gtime = 0.0;
    double d0 = 0.0;  // GOAL: the distance to the goal the branch starts from
    if (running) {
        const double2 p = P.pos[g0], v = P.vel[g0], g = P.goal[g0], rv = P.rv[g0];
        px = p.x, py = p.y, vx = v.x, vy = v.y, gx = g.x, gy = g.y, rad = rv.x, vpref = rv.y;
        gtime = P.gtime[b];
        theta = P.theta[b];  // (carried by UNI engines only, reported by all)
        if (GOAL) d0 = norm2(px - gx, py - gy);
    }
    const bool mine = running;
    double cur_return = 0.0;
    int cur_steps = 0, info = CN_NOTHING;
    const double2* const row = reinterpret_cast<const double2*>(action_table) + v_env * (size_t)P.n_steps;
    const cn_lookahead_out O = *Od;
    __syncthreads();

    for (int t = 0; t < P.n_steps; ++t) {
        const double2* const cur = h_pos[t & 1];
        double2* const nxt = h_pos[(t + 1) & 1];
        bool ends = false;
        const int vi = PATHS ? t & 1 : 0, vn = PATHS ? (t + 1) & 1 : 0;  // h_vel's buffer before step t, after it
        if (PATHS && lane < H) {  // the velocity this lane's human chooses at step t
            const double2 v = vel_rows[(size_t)t * (size_t)H + lane];
            hvx = v.x, hvy = v.y;
        }
        if (running) {
            const double2 a = row[t];
            // the transition (transition.h): the robot's step, the slot order scan over the swept distances — the human's CURRENT
            // velocity against the robot's NEW action — and the outcome
            const RobotStep rs = robot_step(UNI, px, py, a.x, a.y, theta, P.dt);
            double dmin = std::numeric_limits<double>::infinity();
            bool collision = false;
            for (int i = 0; i < H; ++i) {
                const double2 hp = cur[i], hv = h_vel[vi][i];
                const double2 cp = closest_point(hp.x - px, hp.y - py, hv.x - rs.vx, hv.y - rs.vy, P.dt);
                const double c = norm2(cp.x, cp.y) - h_rv[i].x - rad;
                dmin = scan_dmin(dmin, collision, c);
                collision = scan_collision(collision, c);
            }
            const bool reaching = norm2(rs.ex - gx, rs.ey - gy) < rad;
            const Outcome o = outcome_of(gtime >= P.time_limit - 1.0, collision, reaching, dmin, P.success_reward, P.collision_penalty,
                                         P.discomfort_dist, P.discomfort_factor, P.dt);
            info = o.info, ends = o.done;
            // the book (CN_BOOK_TRANSITION; a running branch has made t transitions) and the clock
            const double disc = (t < kMaxDiscount && t < P.discount_len) ? P.discount[t] : 0.0;
            cur_return = cur_return + disc * o.reward;
            ++cur_steps;
            gtime += P.dt;
            // Agent.step
            px = rs.ex, py = rs.ey;
            const RobotAfter ra = robot_after(UNI, a.x, rs.th, rs.vx, rs.vy, theta);
            vx = ra.vx, vy = ra.vy, theta = ra.theta;
            ends = ends || t == P.n_steps - 1;
        }
        // the humans' move of this step, by the lane that owns each: one multiply and one add per coordinate
        if (lane < H) {
            hx = hx + hvx * P.dt;
            hy = hy + hvy * P.dt;
            nxt[lane] = make_double2(hx, hy);
            if (PATHS) h_vel[vn][lane] = make_double2(hvx, hvy);
        }
        if (ends) running = false;
        const int any_running = __syncthreads_or(running ? 1 : 0);  // ... and nxt is written
        if (ends && O.final_state8) {  // cn_get_state's rows of branch (b, k): the state after its last transition
            double2* dst = reinterpret_cast<double2*>(O.final_state8) + v_env * (size_t)P.A * 4;
            dst[0] = make_double2(px, py), dst[1] = make_double2(vx, vy);
            dst[2] = make_double2(gx, gy), dst[3] = make_double2(rad, vpref);
            for (int i = 0; i < H; ++i) {
                dst += 4;
                dst[0] = nxt[i], dst[1] = h_vel[vn][i], dst[2] = h_goal[i], dst[3] = h_rv[i];
            }
        }
        if (!any_running) break;
    }
    if (mine) {
        O.ret[v_env] = GOAL ? cur_return + goal_weight * (d0 - norm2(px - gx, py - gy)) : cur_return;
        O.info[v_env] = (uint8_t)info;
        O.steps[v_env] = cur_steps;
        O.time[v_env] = gtime;
        if (O.final_theta) O.final_theta[v_env] = theta;
    }
