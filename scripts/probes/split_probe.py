"""What the two waves of the two-wave fused rollout kernel do per step, and how long each waits for the other.
(profiling build: make -C crowdnav_amd/csrc exp NAME=probe DEFS=-DCN_SPLIT_PROBE EXP_TU=env;
 CROWDNAV_AMD_LIB=build/exp/lib_probe.so [CROWDNAV_AMD_SPLIT_ASSIST=0|1] python scripts/probes/split_probe.py [envs] [steps])
Per launch, summed over the workgroups: iterations of the ORCA wave's loop, redone iterations (one per episode end of a
workgroup), steps that took the 3-D fallback, iterations with the third barrier (the env wave ran the fallback's head), head
hits / misses / false alarms (with the switch at 0 no head exists, so every fallback step counts as a miss), and the
shader-clock ticks each wave spent in barriers 1 / 2 / 3 — the wait at barrier 1, where window 2 of the previous iteration
ends, also by what that iteration was: its step took the fallback / it had the third barrier."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import crowdnav_amd  # noqa: E402
from crowdnav_amd import _lib  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
lib = _lib.load()
probe = lib.cn_debug_split_probe
probe.restype, probe.argtypes = C.c_int, [C.c_void_p, C.c_int]
eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=crowdnav_amd.ROBOT_ORCA, robot_visible=1)
assert eng.rollout_route(N) == 'fused_split', eng.rollout_route(N)
eng.rollout_begin(seed_base=2000, seed_mod=2 ** 32 - 2000, record_capacity=1)
eng.rollout(200)
eng.sync()
assert probe(None, 1) == 0
print('CROWDNAV_AMD_SPLIT_ASSIST=%s, %d envs' % (os.environ.get('CROWDNAV_AMD_SPLIT_ASSIST', '(default)'), B))
for n in (N, N, 20):
    eng.rollout(n)
    eng.sync()
    out = (C.c_ulonglong * 32)()
    assert probe(out, 1) == 0
    it, redo, fb, head, hit, miss, alarm = [int(out[k]) for k in range(7)]
    wg = (B + 1) // 2
    print('%5d steps: %d iterations of %d workgroups, redone %.4f per workgroup-step' % (n, it, wg, redo / (wg * n)))
    print('      since the engine was created (fresh_starts): %s' % eng.fresh_starts())
    print('      per iteration: fallback %.4f   third barrier %.4f   hit %.4f   miss %.4f   false alarm %.4f'
          % tuple(x / it for x in (fb, head, hit, miss, alarm)))
    print('      ticks in barriers per iteration:  ORCA wave 1: %.0f  2: %.0f  3: %.0f (per third barrier: %.0f)   '
          'env wave 1: %.0f  2: %.0f  3: %.0f (per third barrier: %.0f)'
          % (out[7] / it, out[8] / it, out[9] / it, out[9] / max(head, 1), out[10] / it, out[11] / it, out[12] / it,
             out[12] / max(head, 1)))
    for w, name in ((0, 'ORCA wave'), (1, 'env wave ')):
        b = 13 + 4 * w
        n_fb, n_hd = int(out[b + 2]), int(out[b + 3])
        all1 = int(out[7 + 3 * w])
        print('      %s at barrier 1, per iteration: behind a fallback step %.0f (%d)   behind any other %.0f   behind a third-barrier '
              'iteration %.0f (%d)   behind any other %.0f'
              % (name, out[b] / max(n_fb, 1), n_fb, (all1 - int(out[b])) / max(it - n_fb, 1), out[b + 1] / max(n_hd, 1), n_hd,
                 (all1 - int(out[b + 1])) / max(it - n_hd, 1)))
