// When the scenario ring of the lane-per-scenario generator is filled: the host's rule, stated once.  Plain C++ (nothing of
// HIP is included), so that a CPU program can run it: tests/test_fill_plan_host.py brute-forces the invariants below.
//
// The ring holds C slots per env; ordinal o lives in slot o % C.  A launch of n transitions may look D scenarios ahead of
// the env's next ordinal, never further (CN_LOAD_EPISODE clamps the stored fill level to next + D), so an env consumes at
// most m = min(n, D) scenarios per call.  C == D is the synchronous ring: every fill runs on the engine's stream in front
// of the launch that needs it.  C == 2 D is the lagged ring: a fill tops the ring up to next + C, which pays for TWO calls'
// worth of consumption, and the top-up for the call after the next one runs on a side stream BESIDE the launch in between.
//
// `ahead` is a lower bound on (stored fill level - next ordinal) of every env at the start of the next call.  `since` is
// the synchronous rule's own counter (transitions launched since its last fill), kept in both modes: where that rule fills,
// its launch sees level = next + D exactly, and so must this one (need() = D there); where it does not, the call's n
// transitions are inside its budget and any level >= next + n gives the same rollout (need() = n).
//   D = 48, calls of 30, 30, 30 steps show why `since` is kept: after the first call's fill to next + 96 the third call
//   has ahead = 36 >= 30 and would never run dry, but its launch would see next + 36 where the synchronous rule, which
//   fills in front of it, shows next + 48.  With need() = D a fill runs beside the second call, and the third sees next + 48.
//
// The ring has TWO level buffers.  A launch reads one; a fill — in front of the launch or beside it — reads the same one and
// writes the other, and the two change hands ONCE per fill: at once for a fill in front, and for a fill beside a launch when
// its levels are taken — by the next call (Decision::take_levels: that launch first waits for the fill) or by a settle()
// between the calls, whichever comes first.  `pending` is that fill: enqueued, its levels taken by nobody yet.
#pragma once

namespace cn {

struct FillPlan {
    int D = 1, C = 1;  // scenarios a launch may look ahead; slots per env (D, or 2 D with the lagged fill)
    int ahead = -1;    // < 0: nothing is known about the ring (cn_rollout_begin)
    int since = -1;    // the synchronous rule's transitions since its last fill; < 0: never filled
    bool pending = false;  // a fill beside the previous launch wrote levels that no launch has taken yet

    struct Decision {
        bool sync_fill;    // fill on the engine's stream, in front of the launch
        bool lagged_fill;  // fill on the side stream, beside the launch (ordered behind everything in front of it)
        bool take_levels;  // first of all: wait for the fill beside the previous launch and take the levels it wrote
    };

    void configure(int depth, bool lagged) { D = depth < 1 ? 1 : depth, C = lagged ? 2 * D : D, begin(); }
    void begin() { ahead = -1, since = -1; }
    bool lagged() const { return C > D; }
    bool sync_rule_fills(int n) const { return since < 0 || since + n > D; }
    // scenarios ahead of every env that a launch of n transitions must find
    int need(int n) const { return sync_rule_fills(n) ? D : n; }
    // Between two calls, before anything outside a rollout reads or writes what a fill beside the previous launch reads or
    // writes (env state, the io block, the ring's bookkeeping).  True: one is out — wait for it, then take its levels.  What
    // the next call decides and what its launch sees do not depend on whether a settle came first.
    bool settle() {
        const bool take = pending;
        pending = false;
        return take;
    }

    // One call of n >= 1 transitions: what to enqueue around its launch.
    Decision call(int n) {
        const int m = n < D ? n : D;
        Decision d{ahead < need(n), false, settle()};
        if (d.sync_fill) ahead = C;  // level = next + C of every env
        since = sync_rule_fills(n) ? n : since + n;
        ahead -= m;  // the launch consumes at most m
        // would a repeat of this call need a fill?  Then it runs beside this one.  It reads each env's (state, episodes
        // finished) word before or after that env's workgroup of this launch stores it: level >= (next before this launch)
        // + C >= (next after it) + C - m either way.
        if (lagged() && ahead < need(n)) d.lagged_fill = pending = true, ahead = C - m;
        return d;
    }
};

}  // namespace cn
