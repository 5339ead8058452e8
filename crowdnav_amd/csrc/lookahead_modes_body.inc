// The lane body of lookahead_modes_kernel and lookahead_modes_goal_kernel (lookahead_modes_kernel.h, whose header describes it).
// Included text, not a __device__ function, for lookahead_cv_body.inc's reason.  In scope where it is included: UNI, GOAL
// (constexpr bool), P (CvParams), action_table, Q (ModesParams), goal_weight (0.0 without GOAL).
// GOAL = true (include/crowdnav_amd.h, "Lookahead goal-progress term"): the robot moves once for the M modes, so d0 is taken once
// where the robot row is loaded and d1 once per step, from the step's end point — the robot's position after that step.  A mode's
// book gets goal_weight * (d0 - d1) at the step the mode ends: its own done, a Timeout or ReachGoal that ends every running mode,
// or the horizon.  The reduction behind the loop then runs on those returns.
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
    const double d0 = GOAL ? norm2(px - gx, py - gy) : 0.0;  // the distance to the goal every mode starts from
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
            const double d1 = norm2(rs.ex - gx, rs.ey - gy);  // the distance to the goal after this step
            const bool reaching = d1 < rad;
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
                    if (o.done || last) {
                        running &= ~(1u << m);
                        if (GOAL) m_ret[m] = m_ret[m] + goal_weight * (d0 - d1);
                    }
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
