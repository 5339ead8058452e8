// The body of rollout_kernel, rollout_trace_kernel and the two rollout_actions kernels (rollout_kernels.h), included once into
// each: one source, four kernels.
// In scope where it is included: MAXL, UNI, HEADLINE, KD (compile-time), P_in, Sd, ring_filled_in, R, n_steps, ext_action,
// and under CN_ROLLOUT_TRACE the caller's cn_trace_out T.  Under CN_ROLLOUT_ACTIONS the call's action table
// action_table (double [B][n_steps][2]) takes the place of ext_action.  Under CN_ROLLOUT_LOOKAHEAD (with CN_ROLLOUT_ACTIONS;
// rollout_lookahead_kernel) the envs are the B K virtual ones of a cn_lookahead_actions call: P_in.B = B K, n_candidates = K,
// Od the device copy of the caller's cn_lookahead_out; ring_filled_in and R.io are not in scope / not read; GOAL (constexpr bool)
// says whether ret carries the goal-progress term, whose weight then lies behind *Od.
// Why an include and not a __device__ __forceinline__ template with a TRACE parameter: with the body behind a call, its
// arguments passed by value or by reference alike, hipcc gave every existing rollout_kernel instantiation a different
// instruction stream (a hundred instructions more or fewer each, the 20-human shard's kernel included).  Included text leaves
// rollout_kernel the tokens it had, hence the code it had (scripts/kernel_asm_diff.py).
    // The ~20 state pointers are needed before and after the step loop and when an episode ends, never inside a step: they
    // are re-read from the engine's device copy of the StateView there (scalar loads) instead of holding 40 SGPRs — spilled
    // into VGPR lanes, and at 10 half-planes pushing vector registers into scratch — across the loop.  ring_filled_in is the
    // one pointer the host swaps between launches (fill_ring_if_needed), hence a direct argument.
    // HEADLINE: the geometry of BASELINE configs[1] (5 humans + robot, 2 envs per 64-lane workgroup) as compile-time
    // constants — the pair loops become single passes, the 5-candidate rank loop unrolls, divisions by A / NC fold:
    // 706 -> 740 M env-steps/s.  Every other geometry runs the generic instantiation.
    Params P = P_in;
    if (HEADLINE && MAXL == 5) {
        P.A = 6, P.NC = 5, P.E = 2, P.nA = 12, P.pairs = 60, P.threads = 64;
    }
    if (HEADLINE && MAXL == 10) {  // BASELINE configs[3]'s shard: 20 humans + robot, one env per 64-lane workgroup, 10 neighbours
        // kept of 20 candidates — every LDS offset an immediate, no scalar registers for the layout (the generic instantiation
        // spills 200+ SGPRs into VGPR lanes)
        P.A = 21, P.NC = 20, P.E = 1, P.nA = 21, P.pairs = 420, P.threads = 64, P.kd = KD ? 1 : 0;
        P.orca.max_neighbors = 10;
        P.kdl = kd_layout(21, 21, 1);
    }
    constexpr bool COMPACT = HEADLINE && MAXL == 10;  // the shard kernel's LDS layout (carve)
    // the float64 parameters of a step as VALU operands live in VGPRs (rollout_fused.h: in_vgpr): as SGPR kernel arguments the
    // 16-dword block was spilled into VGPR lanes and re-read with v_readlane several times per step (COMPACT: in LDS instead)
    if (!COMPACT) {
        auto pin = [](double& x) { asm volatile("" : "+v"(x)); };
        pin(P.dt), pin(P.time_limit), pin(P.success_reward), pin(P.collision_penalty), pin(P.discomfort_dist);
        pin(P.discomfort_factor), pin(P.human_safety);
    }
    // The shard's kernel is compiled for three resident waves per SIMD: 3072 workgroups fill the chip, 4096 envs would run as
    // a full round and a third of one.  launch_rollout therefore splits a call of 3 q steps into FOUR launches of q steps over
    // 3 B / 4 workgroups: sub-launch k leaves out env 3 - k of every group of four (ABC, ABD, ACD, BCD), so every env makes
    // its 3 q steps, in order, and every launch is exactly one round of the chip.
    int env_block = -1, extra_env = -1;
    if (HEADLINE && MAXL == 10 && P.sched >= 0) {
        const int g = (int)blockIdx.x / 3, rr = (int)blockIdx.x - 3 * g, skip = 3 - P.sched;
        env_block = 4 * g + rr + (rr >= skip ? 1 : 0);
        if (P.sched == 3 && rr == 0) extra_env = 4 * g;  // the last sub-launch reports for the env it leaves out as well
    }
    const Smem s = carve<MAXL, COMPACT>(P);
    if (COMPACT && threadIdx.x == 0) {
        s.disc[kParDt] = P.dt, s.disc[kParLimit] = P.time_limit, s.disc[kParSuccess] = P.success_reward;
        s.disc[kParCollision] = P.collision_penalty, s.disc[kParDDist] = P.discomfort_dist;
        s.disc[kParDFactor] = P.discomfort_factor, s.disc[kParHSafety] = P.human_safety;
    }
    constexpr bool kDyn = HEADLINE && MAXL == 10;
    const bool dynamic = kDyn && P.sched == kSchedDynamic;
    if (kDyn && threadIdx.x == 0) reinterpret_cast<EpisodeLds*>(s.disc + 8)->dyn_total = 0u;
    const int n_steps_call = n_steps;
    for (int visit_iter = 0; dynamic || visit_iter == 0; ++visit_iter) {
    int dyn_env = 0, dyn_k = 0;
    if (kDyn && dynamic) {
        __syncthreads();  // (the previous visit's last LDS reads are done)
        if (threadIdx.x == 0) {
            int* const queue = Sd->dyn_queue;
            const int v = atomicAdd(queue, 1);
            if (v < P.dyn_visits * P.B) {  // wait for the env's previous visit: its state is in memory once the flag says so
                const int env = v % P.B, k = v / P.B;
                int spins = 0;
                while (__hip_atomic_load(queue + 1 + env, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < k && spins < (1 << 22)) {
                    __builtin_amdgcn_s_sleep(16);
                    ++spins;
                }
                // ~2 s: never in a healthy run; cn_sync reports it.  The visit is then NOT run on state its predecessor may still
                // be writing (ADVICE r5): it is handed on as if complete, so that the env's later visits do not wait in turn —
                // the env loses those steps, the error bit says so
                if (spins == (1 << 22)) {
                    atomicOr(Sd->error, 4);
                    __hip_atomic_store(queue + 1 + env, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    s.flag[2] = 1;
                } else {
                    s.flag[2] = 0;
                }
            }
            s.flag[1] = v;
        }
        __syncthreads();
        const int v = s.flag[1];
        if (v >= P.dyn_visits * P.B) break;
        if (s.flag[2] != 0) continue;  // (the wait gave up)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every wave: what the previous visit's workgroup wrote is visible
        dyn_env = v % P.B, dyn_k = v / P.B;
        env_block = dyn_env;
        const int q = n_steps_call / P.dyn_visits, rem = n_steps_call - q * P.dyn_visits;
        n_steps = q + (dyn_k < rem ? 1 : 0);
    }
    const Lane L = lane_of(P, env_block);
    AgentRegs r = {};
    float robot_max_speed = 0.0f;
    const bool robot = L.valid && L.a == 0;
    double theta = 0.0;  // heading of a unicycle robot (external actions only)
    EpisodeBook ep = {};  // (state = kRetired)
#ifdef CN_ROLLOUT_LOOKAHEAD
    // L is the lane of VIRTUAL env v = b K + k (P.B = B K): the action row, the outputs and which lanes exist go by it.  What
    // the branch starts from is env b = v / K of the engine, read through Lsrc and never written: agents, heading, kd rows,
    // global time.  Two envs of one workgroup may have different sources (K odd), each lane divides for itself.
    {
        const StateView S = *Sd;
        Lane Lsrc = L;
        Lsrc.env = L.env / n_candidates;
        Lsrc.gi = (size_t)Lsrc.env * (size_t)P.A + (size_t)L.a;
        if (L.valid) load_agent(S, Lsrc.gi, r);
        if (KD) kd_load(P, S, s, Lsrc);
        if (robot) {
            theta = S.theta[Lsrc.env];
            ep.gtime = S.gtime[Lsrc.env];  // a fresh book: cur_* = 0, the discount index starts at 0
            ep.state = kRunning;
            s.flag[L.lane] = 1;
        }
    }
    int look_info = CN_NOTHING;  // (robot lane) info code of the last transition made
    if (visit_iter == 0) build_pairs<COMPACT>(P, s, dynamic);
    __syncthreads();
#else
    {
        const StateView S = *Sd;
        if (L.valid) load_agent(S, L.gi, r);
        if (P.robot_orca) load_robot_view(P, S, s, L, r, robot_max_speed);
        if (KD) kd_load(P, S, s, L);
        if (robot) theta = S.theta[L.env];
    }
    if (visit_iter == 0) build_pairs<COMPACT>(P, s, dynamic);
    if (robot) {
        const StateView S = *Sd;
        const cn_rollout_io io = *R.io;
        CN_LOAD_EPISODE(P, ep, S, io, ring_filled_in, L.env);
        int f = ep.state == kRunning ? 1 : 0;
        if (ep.state == kWaitingScenario && scenario_ready(P, S, L.env, ep.ep_count, ep.ring_filled)) {  // produced since
            f = 2 + ep.ep_count % P.ring_mod;
            ep.state = kRunning;
            ep.gtime = 0.0;
        }
        s.flag[L.lane] = f;
    }
    __syncthreads();
    if (L.valid && s.flag[L.ebase] >= 2) {
        load_from_ring(P, *Sd, L, s.flag[L.ebase] - 2, r);
        if (KD) kd_new_episode(P, s, L);
        theta = 1.5707963267948966;
    }
#endif
    // COMPACT: what an agent keeps for a whole episode goes to LDS here and whenever the env loads its next scenario
    const auto stage_constants = [&]() {
        if (L.lane < P.nA) {
            s.goal2[L.lane] = make_double2(r.gx, r.gy);
            s.vpref[L.lane] = r.vpref;
            s.rad[L.lane] = r.rad;
            s.hview[L.lane] = (float)(r.rad + 0.01 + P.human_safety);
        }
    };
    if (COMPACT) stage_constants();
    unsigned int transitions = 0;
    if (!COMPACT)
        for (int t = threadIdx.x; t < kMaxDiscount; t += blockDim.x) s.disc[t] = t < R.discount_len ? R.discount[t] : 0.0;
    // COMPACT: the robot lane's episode bookkeeping waits in LDS while a transition is computed (12 VGPRs the step loop
    // does not hold across the pair and solve phases); `ep` is its copy in registers while a transition is booked
    EpisodeLds* const eps = reinterpret_cast<EpisodeLds*>(s.disc + 8);
    if (COMPACT && robot) eps->book = ep, eps->transitions = 0u;
    __syncthreads();
    const int disc_len = R.discount_len < kMaxDiscount ? R.discount_len : kMaxDiscount;

#ifdef CN_PHASE_TIMING
    PhaseClock clock = {};
    PhaseClock* clk = &clock;
    clock.last = __builtin_readcyclecounter();
#else
    PhaseClock* clk = nullptr;
#endif
    for (int step = 0; step < n_steps; ++step) {
        // The lane ids of this step are opaque to the compiler: everything derived from them — LDS addresses of every phase —
        // is recomputed in the step instead of being hoisted out of the step loop and held in VGPRs across it (step_kernel,
        // the same code without the loop, needs 92 VGPRs; this kernel needed 182 before).
        Lane Ls = L;
        asm volatile("" : "+v"(Ls.lane), "+v"(Ls.a), "+v"(Ls.ebase));
        Ls.valid = L.valid && s.flag[L.ebase] != 0;  // env is running

#ifdef CN_ROLLOUT_TRACE
        size_t trace_row = 0;
        {
            // [B][n_steps] rows; an env's agents are 64 A contiguous bytes of state8 per step, four 16-byte stores per lane
            trace_row = (size_t)L.env * (size_t)n_steps_call + (size_t)step;
            if (Ls.valid) {
                double2* const dst = reinterpret_cast<double2*>(T.state8 + (trace_row * (size_t)P.A + (size_t)L.a) * 8);
                dst[0] = make_double2(r.px, r.py), dst[1] = make_double2(r.vx, r.vy);
                dst[2] = make_double2(r.gx, r.gy), dst[3] = make_double2(r.rad, r.vpref);
            }
            if (robot) {
                T.episode[trace_row] = ep.state == kRunning ? ep.ep_count : -1;  // -1: retired, or waiting for its next scenario
                if (ep.state == kRunning) T.step[trace_row] = ep.cur_steps;
            }
        }
#endif

#ifdef CN_ROLLOUT_ACTIONS
        // step_core reads the robot lane's action at ext_action[2 * env]: from this base that is action_table[env][step].  Only
        // the robot lane of a running env reads it (a retired or waiting env ignores its row); the other lanes form no address
        // outside the table.
        const double* const ext_action =
            robot ? action_table + 2 * ((size_t)L.env * (size_t)(n_steps_call - 1) + (size_t)step) : action_table;
#endif
        StepResult res;
        double nvx, nvy;
        if constexpr (COMPACT) {
            // The book lives in LDS (eps->book) and comes into registers field by field, for the bookkeeping only: what every
            // transition touches (`e`), and episodes finished / fill level / state at an episode end alone.  No LDS copy of the
            // discount table either: this step's factor is requested here, a whole transition before its use, with global_time.
            // (The whole book copied in and out, as one struct, cost the shard's kernel 1.9 %: profiles/episode_book_refactor.txt)
            EpisodeBook& book = eps->book;
            double disc_now = 0.0, gt = 0.0;
            if (robot) {
                const int cs = book.cur_steps;
                gt = book.gtime;
                if (cs < disc_len) disc_now = R.discount[cs];
            }
            step_core<MAXL, UNI, KD, true>(P, s, Ls, r, gt, robot_max_speed, ext_action, 1, res, nvx, nvy, &theta, clk);
            if (robot && book.state == kRunning) {
                int next_flag = 1;
                EpisodeBook e;
                e.cur_steps = book.cur_steps, e.cur_danger = book.cur_danger;
                e.cur_return = book.cur_return, e.cur_dsum = book.cur_dsum;
                e.gtime = gt;
                eps->transitions += 1u;
                CN_BOOK_TRANSITION(e, disc_now, res.reward, res.info, res.dmin);
                if (res.done) {
                    e.ep_count = book.ep_count, e.ring_filled = book.ring_filled, e.state = kRunning;
                    const cn_rollout_io io = *R.io;
                    next_flag = 0;
                    CN_END_EPISODE(P, *Sd, io, L.env, true, s.disc[kParLimit], res.info, e, next_flag = 2 + e.ep_count % P.ring_mod);
                    book.ep_count = e.ep_count, book.state = e.state;
                }
                book.gtime = e.gtime;
                book.cur_steps = e.cur_steps, book.cur_danger = e.cur_danger, book.cur_return = e.cur_return, book.cur_dsum = e.cur_dsum;
                s.flag[L.lane] = next_flag;
            }
        } else {
            step_core<MAXL, UNI, KD>(P, s, Ls, r, ep.gtime, robot_max_speed, ext_action, 1, res, nvx, nvy, &theta, clk);
            if (robot && ep.state == kRunning) {
                int next_flag = 1;
                ++transitions;
#ifdef CN_ROLLOUT_TRACE
                if (T.reward) T.reward[trace_row] = res.reward;
                if (T.info) T.info[trace_row] = res.info;
                if (T.dmin) T.dmin[trace_row] = res.dmin;
#endif
                const double disc = ep.cur_steps < kMaxDiscount ? s.disc[ep.cur_steps] : 0.0;
                CN_BOOK_TRANSITION(ep, disc, res.reward, res.info, res.dmin);
#ifdef CN_ROLLOUT_LOOKAHEAD
                look_info = res.info;
                if (res.done) next_flag = 0, ep.state = kRetired;  // the branch ends here: its lanes keep what they hold
#else
                if (res.done) {  // 0 = the env stops stepping (retired, or waiting for its scenario), 2 + slot = every lane loads it
                    const cn_rollout_io io = *R.io;
                    next_flag = 0;
                    CN_END_EPISODE(P, *Sd, io, L.env, true, P.time_limit, res.info, ep, next_flag = 2 + ep.ep_count % P.ring_mod);
                }
#endif
                s.flag[L.lane] = next_flag;
            }
        }
#ifdef CN_ROLLOUT_LOOKAHEAD
        // (no next scenario to load; a workgroup whose branches have all ended has nothing left to step)
        if (!__syncthreads_or(robot && ep.state == kRunning ? 1 : 0)) break;
#else
        __syncthreads();
        if (L.valid && s.flag[L.ebase] >= 2) {
            load_from_ring(P, *Sd, L, s.flag[L.ebase] - 2, r);
            if (KD) kd_new_episode(P, s, L);
            theta = 1.5707963267948966;  // robot.set(..., np.pi / 2)
            if (COMPACT) stage_constants();
        }
#endif
        CN_TICK(clk, 7);
    }
    if (COMPACT && L.lane < P.nA) {
        const double2 g = s.goal2[L.lane];
        r.gx = g.x, r.gy = g.y, r.vpref = s.vpref[L.lane], r.rad = s.rad[L.lane];
    }
    if (COMPACT && robot) ep = eps->book, transitions = eps->transitions;
#ifdef CN_PHASE_TIMING
    if ((threadIdx.x & (kWave - 1)) == 0) {
        for (int k = 0; k < 10; ++k) atomicAdd(&cn_phase_cycles[k], clock.acc[k]);
        atomicAdd(&cn_phase_cycles[15], 1ull);  // waves
    }
#endif

#ifdef CN_ROLLOUT_LOOKAHEAD
    // Nothing of the engine is written: no agent state, no book, no kd rows, no epilogue.  A stopped env's lanes were not
    // stepped again (Ls.valid), so the registers hold the state after each branch's LAST transition, ended or still running:
    // one store per output here instead of one at the episode end and one behind the loop.  The six pointers come from the
    // device copy of the caller's block, as the state pointers do: no register of the step loop holds them.
    {
        const cn_lookahead_out O = *Od;
        if (robot) {
            double ret = ep.cur_return;
            if (GOAL) {
                // rollout_lookahead_goal_kernel (include/crowdnav_amd.h, "Lookahead goal-progress term").  Nothing of the term is
                // held across the step loop: as a kernel argument the weight — or d0 in two registers — sent the kd
                // instantiations to scratch where their plain forms have none (profiles/lookahead_goal_kernels.txt).  So the
                // weight is read here from behind the device copy of the caller's block, whose pointer the tail needs anyway
                // (upload_look_goal puts it there), and d0 from the robot's start row, read AGAIN from the source env the
                // prologue read it from and nothing has written.  d1: r.px, r.py are the position final_state8 reports
                // below.  One subtraction, one multiply, one add.
                const double goal_weight = *reinterpret_cast<const double*>(Od + 1);
                const double2 p0 = Sd->pos[(size_t)(L.env / n_candidates) * (size_t)P.A];
                ret = ret + goal_weight * (norm2(p0.x - r.gx, p0.y - r.gy) - norm2(r.px - r.gx, r.py - r.gy));
            }
            O.ret[L.env] = ret;
            O.info[L.env] = (uint8_t)look_info;
            O.steps[L.env] = ep.cur_steps;
            O.time[L.env] = ep.gtime;
            if (O.final_theta) O.final_theta[L.env] = theta;
        }
        if (L.valid && O.final_state8) {  // cn_get_state's row of virtual env v: [v][a][8]
            double2* const dst = reinterpret_cast<double2*>(O.final_state8 + L.gi * 8);
            dst[0] = make_double2(r.px, r.py), dst[1] = make_double2(r.vx, r.vy);
            dst[2] = make_double2(r.gx, r.gy), dst[3] = make_double2(r.rad, r.vpref);
        }
    }
    (void)transitions, (void)extra_env;
    }  // visits
#else
    const StateView S = *Sd;
    if (KD) kd_store(P, S, s, L);
    if (L.valid) CN_STORE_AGENT(S, L.gi, r);
    if (robot) {
        const cn_rollout_io io = *R.io;
        CN_STORE_EPISODE(P, S, io, L.env, ep, theta);
    }
    if (kDyn && dynamic) {
        if (robot) {
            const cn_rollout_io io = *R.io;
            if (io.env_transitions) io.env_transitions[L.env] += (uint64_t)transitions;
            eps->dyn_total += transitions;
        }
        // release: this env's state, bookkeeping and kd rows are in memory before its next visit may start anywhere
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(Sd->dyn_queue + 1 + dyn_env, dyn_k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        continue;
    }
    rollout_epilogue(P, S, *R.io, L, robot, transitions, ep.ep_count, reinterpret_cast<double*>(s.lines), extra_env);
    }  // visits
    if (kDyn && dynamic) {
        // the job-wide transitions counter, if the caller keeps one (per-env counters were added visit by visit; the in-kernel
        // summary / record blocks are not offered under the dynamic schedule: launch_rollout falls back to the static one)
        __syncthreads();
        cn_rollout_io io = *R.io;
        io.blocks = nullptr, io.summary = nullptr, io.env_transitions = nullptr;
        Lane Le;
        Le.lane = threadIdx.x, Le.env = (int)blockIdx.x, Le.a = threadIdx.x == 0 ? 0 : 1, Le.ebase = 0, Le.valid = true, Le.gi = 0;
        const unsigned int dyn_transitions = threadIdx.x == 0 ? reinterpret_cast<EpisodeLds*>(s.disc + 8)->dyn_total : 0u;
        rollout_epilogue(P, *Sd, io, Le, threadIdx.x == 0, dyn_transitions, 0, reinterpret_cast<double*>(s.lines));
    }
#endif
