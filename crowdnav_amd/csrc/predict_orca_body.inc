// The body of predict_orca_kernel and predict_orca_robot_kernel (predict_orca_kernel.h), included into each: kernel text, so that
// the robot-unseen kernels are compiled from exactly the statements they had before there was a second one (a shared
// __forceinline__ function over `const Params&` did change their instruction streams).  The including kernel provides MAXL, KD,
// P, S, n_steps, n_modes, mode, human_vel and the constants ROBOT, UNI; with ROBOT also robot_actions and env_stride.
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
    const bool robot = ROBOT && L.valid && L.a == 0;
    double theta = 0.0;
    const double* arow = robot_actions;
    if (ROBOT && robot) {
        arow = robot_actions + 2 * (size_t)L.env * (size_t)env_stride;
        if (UNI) theta = S.theta[L.env];
    }
    for (int t = 0; t < n_steps; ++t) {
        double2 act = make_double2(0.0, 0.0);
        if (ROBOT && robot) act = make_double2(arow[2 * (size_t)t], arow[2 * (size_t)t + 1]);  // used behind the solve
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
        if (ROBOT && robot) {  // Agent.step of an external robot: the row as given, not clipped
            const RobotStep rs = robot_step(UNI, r.px, r.py, act.x, act.y, theta, P.dt);
            const RobotAfter ra = robot_after(UNI, act.x, rs.th, rs.vx, rs.vy, theta);
            r.px = rs.ex, r.py = rs.ey;
            r.vx = ra.vx, r.vy = ra.vy;
            theta = ra.theta;
        }
        block_sync(P);  // the solve's last LDS reads, before the next step's stage phase writes
    }
