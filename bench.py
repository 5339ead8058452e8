"""bench.py — env-steps/sec of the batched ORCA step (BASELINE.json metric) on N MI355X GPUs of one node.

A "step" is one transition of EVERY env of the batch (4096 envs x 5 humans per GPU, ORCA humans + holonomic
ORCA robot, in-kernel auto-reset): `--steps K` executes exactly K such batched steps per rank after W warm-up
steps, in fused launches of at most `--chunk` steps each.  value = total env transitions of all ranks / wall time.

    python bench.py                                        # 1 GPU: the headline only
    python bench.py --full                                 # + everything measured beside it (see below)
    python bench.py --dump-outputs DIR                     # + what the timed steps computed, as DIR/<name>.npy
    python bench.py --gpus N [--steps K --warmup W]        # N GPUs: re-executes itself as N ranks (127.0.0.1 rendezvous)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W             # the same under an external launcher (RANK/WORLD_SIZE set)

Before the warm-up every rank runs `--preroll` UNTIMED steps (default 200, stated in config.preroll_steps): all envs
start their first episode in lock step, so without it a short run would time a synchronised batch in which no episode
ends; after it the episodes are spread over all phases and the timed steps contain their share of episode ends and
auto-resets (`episodes_finished`).

The timed region is the step path: the K batched steps — transitions, in-kernel auto-resets, the per-episode records and the
per-env transition counters.  The env axis is sharded over the GPUs (weak scaling: 4096 envs per GPU, global env ids offset
by rank, no collective on the step path); every rank times its own K steps between a barrier + synchronize on both sides,
value = all ranks' transitions / the slowest rank's time.  What a run does ONCE when it ends — the job-wide statistics of
explorer.py:74-90 (the reference computes them after its episode loop), i.e. the record blocks of every shard, on several GPUs
their all-gather (RCCL), and the summary kernel — is the shard boundary: timed separately as `boundary_ms` AT EVERY WORLD SIZE,
1 included (and `value_incl_boundary` charges it to these K steps).  The JSON line also carries
`roofline` (algorithmic bytes of the dominant kernel over its HIP-event duration), `issue_roofline` (the bound that
actually limits this kernel, only when the committed PMC profile is of the same launch shape).  A plain run stops there.
`--full` adds what takes measurements of its own: `value_r3_definition` (a second engine), `fill_ms`, `value_samples` and, at
N=1, `cpu_baseline` (the CPU oracle timed on this host's cores on a bounded sample of the same workload; + the unmodified
reference Python loop as timed in the build container) and `secondary` (BASELINE configs[2] and configs[3] measured in the
same run).  `--dump-outputs DIR` writes the arrays the K timed steps left (env states, episode records and counters, the
boundary's summary) after the run; with the same arguments the inputs are the same seeded episodes from run to run.

Two environment switches exist so that the N > 1 code path can be EXECUTED on a one-GPU box (tests/test_bench_multirank.py):
CROWDNAV_AMD_BENCH_BACKEND=gloo (torch.distributed backend of the ranks; RCCL refuses two ranks on one device, gloo moves
the few collectives of a run through the host) and CROWDNAV_AMD_BENCH_SHARE_GPU=1 (every rank uses device 0).  Numbers
measured that way time two processes sharing one GPU and say nothing about scaling; the line says so (`config.backend`,
`config.shared_gpu`).
"""
import argparse
import contextlib
import gc
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
# 256 CUs x 4 SIMD-32; a wave64 VALU instruction issues over 2 cycles (MI355X_MICROARCH.md: "v_fma_f32 (wave64) 2 cyc")
VALU_ISSUE_PEAK = 1024 * 2.4e9 / 2
PMC_PROFILE = next((p for p in (os.path.join(ROOT, 'profiles', n) for n in ('r06_traffic.json', 'r05_traffic.json'))
                    if os.path.exists(p)), os.path.join(ROOT, 'profiles', 'r06_traffic.json'))
REFERENCE_PYTHON_PROFILE = os.path.join(ROOT, 'profiles', 'r06_reference_python.json')
CONFIG5_PROFILES = [os.path.join(ROOT, 'profiles', n) for n in ('r06_config5_reference_schedule.json',
                                                                 'r05_config5_reference_schedule.json')]


def algorithmic_bytes_per_env_step(H):
    """72 B per agent (read pos/vel/goal/radius/v_pref, write pos/vel) + 26 B per env."""
    return 72 * (H + 1) + 26


def pmc_profile(envs, humans, steps_per_launch, circle_radius=4.0):
    """The committed rocprofv3 PMC record (separate FETCH_SIZE / WRITE_SIZE / SQ passes of this command, per-dispatch
    averages of cn::rollout_kernel) whose launch shape equals the one just timed, or None: counters of a 1000-step
    launch say nothing about a 20-step one."""
    if not os.path.exists(PMC_PROFILE):
        return None
    for rec in json.load(open(PMC_PROFILE)).get('profiles', []):
        if (rec.get('envs'), rec.get('humans'), rec.get('steps_per_launch'), rec.get('circle_radius', 4.0)) == \
                (envs, humans, steps_per_launch, circle_radius):
            return rec
    return None


def pmc_traffic_bytes(rec):
    """HBM bytes per rollout launch; FETCH_SIZE doubled per the gfx950 correction of MI355X_MICROARCH.md §HBM."""
    if rec is None or 'fetch_size_kb' not in rec:
        return None
    return (2 * rec['fetch_size_kb'] + rec['write_size_kb']) * 1024


def pmc_issue(rec, envs, steps_per_launch, launch_seconds):
    """What actually bounds the fused rollout: vector-ALU issue.  SQ_INSTS_VALU per launch (committed PMC pass of the same
    launch shape) over the launch time measured in this run, against 1024 SIMDs x one wave64 VALU instruction per 2 cycles
    at 2.4 GHz.  The peak is for plain f32 instructions: f64 and transcendental instructions issue at half / quarter
    rate, their shares are reported so the reader can discount it."""
    if rec is None or 'sq_insts_valu' not in rec:
        return None
    src = pmc_provenance()
    if src is None or src['stale']:
        return None  # the kernels changed after the counters were collected: no fraction rather than a stale one
    achieved = rec['sq_insts_valu'] / launch_seconds
    out = {'bound': 'valu-issue', 'achieved': achieved / 1e9, 'peak': VALU_ISSUE_PEAK / 1e9,
           'unit': 'G wave-instructions/s', 'frac': achieved / VALU_ISSUE_PEAK,
           'valu_per_env_step': rec['sq_insts_valu'] / (envs * steps_per_launch),
           'counters_from': src, 'note': 'SQ_INSTS_VALU is NOT measured in this run: committed rocprofv3 PMC pass of the same '
                                         'launch shape (counters_from) over the launch time of this run'}
    for k in ('f64_share', 'trans_share', 'lane_occupancy', 'salu_per_valu', 'insts_per_env_step', 'issue_slot_share'):
        if k in rec:
            out[k] = rec[k]
    if 'issue_slot_share' in rec:
        out['issue_slot_note'] = ('round 6 (profiles/r06_valu_rate.txt, measured on this chip): a SIMD takes a plain f32 VALU '
                                  'instruction every 2 cycles, but ONE wave issues an instruction of any class (VALU, SALU, LDS, '
                                  's_waitcnt, s_nop ...) only every ~5 cycles; issue_slot_share = all instructions (SQ_INSTS) x 5 '
                                  'cycles over the waves\' resident cycles — the share of its life a wave spends issuing; the '
                                  'rest it waits for operands.  At 2-3 waves per SIMD that, not the VALU pipe, is what runs out')
    return out


@contextlib.contextmanager
def no_gc():
    """Timed regions run with the cyclic garbage collector off (as timeit does): a generation-2 collection of a process with
    torch loaded takes ~25 ms of HOST time; the launch loop is only a few steps ahead of the GPU right after the opening
    synchronize, so the device drains and idles (r03 kernel trace: one 24 ms hole inside the 50 timed decisions of the third
    measure_sarl of a process, every kernel as fast as before: 2.4 ms per decision read instead of 1.8).  The caller runs
    gc.collect() BEFORE its opening fence: 25 ms of device idle time right in front of the first launch costs the driver shape
    ~100 us of wake-up (20 steps: 251 us instead of 150)."""
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


class Comm:
    """The few collectives of a run (never on the step path): barrier, all-reduce of a handful of float64 scalars, all-gather
    of small Python objects.  backend 'nccl' = RCCL on device tensors; 'gloo' (CROWDNAV_AMD_BENCH_BACKEND, the one-GPU
    execution of this path) stages the scalars through the host."""

    def __init__(self, world, rank, backend):
        self.world, self.rank, self.backend = world, rank, backend

    def barrier(self):
        import torch
        import torch.distributed as dist
        if self.world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def all_reduce(self, values, op='sum'):
        """list of floats -> list of floats, reduced over the ranks"""
        import torch
        import torch.distributed as dist
        if self.world == 1:
            return [float(v) for v in values]
        t = torch.tensor(values, dtype=torch.float64, device='cpu' if self.backend == 'gloo' else 'cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == 'max' else dist.ReduceOp.SUM)
        return [float(v) for v in t.cpu().tolist()]

    def all_gather(self, obj):
        import torch.distributed as dist
        if self.world == 1:
            return [obj]
        out = [None] * self.world
        dist.all_gather_object(out, obj)
        return out


def pmc_provenance():
    """Where issue_roofline's instruction counts come from: the committed PMC profile and the commit that last touched it,
    and whether the kernel sources (crowdnav_amd/csrc) were committed AFTER it — then the counts describe an older kernel
    and the caller drops the field instead of printing a stale fraction.  Outside a git checkout (the GPU box's snapshot
    has no .git) the file's own `csrc_sha` stamp (written by scripts/pmc_to_traffic.py) is compared with the sha256 of the
    sources."""
    rel = os.path.relpath(PMC_PROFILE, ROOT)
    info = {'file': rel, 'stale': False}
    try:
        doc = json.load(open(PMC_PROFILE))
    except (OSError, ValueError):
        return None
    stamp = doc.get('csrc_sha')
    if stamp:
        info['csrc_sha_profiled'] = stamp
        info['stale'] = stamp != csrc_sha()
        return info
    try:
        def last(*paths):
            r = subprocess.run(['git', '-C', ROOT, 'log', '-1', '--format=%H %ct', '--'] + list(paths), capture_output=True,
                               text=True, timeout=10)
            h, t = r.stdout.split()
            return h, int(t)
        (hp, tp), (hc, tc) = last(rel), last(*['crowdnav_amd/csrc/' + n for n in ROLLOUT_SOURCES])
        info['profile_commit'], info['csrc_commit'] = hp[:12], hc[:12]
        info['stale'] = tc > tp
    except Exception:  # no git, no history: cannot tell
        info['stale'] = None
    return info


# the sources of the rollout kernels (what roofline.traffic / issue_roofline describe); the value-network kernels live elsewhere
ROLLOUT_SOURCES = ('kd_order.h', 'orca_device.h', 'rollout_fused.h', 'scenario_device.h', 'scenario_wave.h', 'step_kernels.h')


def csrc_sha():
    """sha256 over the rollout kernels' sources, in name order: identifies the kernels a PMC profile was taken on"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, 'crowdnav_amd', 'csrc')
    for n in ROLLOUT_SOURCES:
        if os.path.exists(os.path.join(d, n)):
            h.update(n.encode())
            h.update(open(os.path.join(d, n), 'rb').read())
    return h.hexdigest()[:16]


def sarl_flop(B, H, om):
    """algorithmic flops of one batched value-network decision: per (env, action) tile of H humans"""
    return 2 * (81 * H * (62050 + (7200 if om else 0)) + 81 * 33500) * B


def measure_sarl(B, H, om, steps, warm, preroll, world, rank, local_rank, comm=None, outputs=None):
    """BASELINE configs[2]: B envs x H humans, SARL value-network rollout (random-init weights), greedy phase.
    A step = cn_sarl_select (81 lookaheads + value network per env) + cn_rollout_step (transition, bookkeeping, seeded
    auto-reset).  HIP events bracket every cn_sarl_select (the MFMA roofline is the value network's flops over THAT time)
    and every whole step.  outputs: a dict that receives what the last timed step computed (host tensors)."""
    import numpy as np
    import torch
    import crowdnav_amd
    from crowdnav_amd import distributed as cd
    from crowdnav_amd.compat.sarl import ValueNetwork, build_action_space
    from crowdnav_amd.sarl_rollout import SarlRollout
    comm = comm or Comm(world, rank, 'nccl')
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL,
                                       robot_visible=1, device=local_rank)
    torch.manual_seed(0)
    net = ValueNetwork(13 + (48 if om else 0), 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)
    space, _, _ = build_action_space(1.0)
    eng.sarl_configure(actions=np.array([[a.vx, a.vy] for a in space]), with_om=om)
    eng.sarl_set_weights(net.state_dict())
    off, stride = cd.shard(rank, world, B)
    ro = SarlRollout(eng, 0.9, seed_base=2000, seed_mod=2 ** 32 - 2000, env_offset=off, env_stride=stride)
    ro.run(preroll)
    ro.run(warm)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    gc.collect()
    for e3 in ev:
        for e in e3:
            e.record()
    torch.cuda.synchronize()
    comm.barrier()
    before = int(ro.transitions.item())
    with no_gc():
        t0 = time.perf_counter()
        for e0, e1, e2 in ev:
            e0.record()
            sel = eng.sarl_select(want_values=False)
            e1.record()
            eng.rollout_step(sel['action'])
            e2.record()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    comm.barrier()
    if outputs is not None:
        state, gtime = eng.get_state()
        outputs.update({k: v.cpu() for k, v in ro.bufs.items()}, best=sel['best'].cpu(), action=sel['action'].cpu(),
                       state=state.cpu(), global_time=gtime.cpu())
    transitions = int(ro.transitions.item()) - before
    per_rank = comm.all_gather({'rank': rank, 'transitions': transitions, 'seconds': elapsed})
    tot = sum(r['transitions'] for r in per_rank)  # real per-rank counts over the slowest rank's time
    tmax = max(r['seconds'] for r in per_rank)
    flop = sarl_flop(B, H, om)
    select_s = sum(a.elapsed_time(b) for a, b, _ in ev) / 1e3 / steps
    step_s = sum(a.elapsed_time(c) for a, _, c in ev) / 1e3 / steps
    name = 'om-sarl' if om else 'sarl'
    out = {
        'metric': 'env-steps/sec, %d envs x %d humans, %s value-net rollout (BASELINE configs[2])' % (B, H, name),
        'value': tot / tmax, 'unit': 'env-steps/s', 'n_gpus': world, 'steps': steps,
        'warmup': warm, 'ms_per_step': tmax * 1e3 / steps, 'higher_is_better': True, 'scaling': 'weak',
        'vs_baseline': None, 'dtype': 'f32 (FP32 MFMA value network, f64 lookahead rewards)', 'data': 'synthetic',
        'config': {'workload': '%d envs x %d humans, 81 actions, %s, random-init weights' % (B, H, name),
                   'preroll_steps': preroll, 'backend': comm.backend if world > 1 else None},
        'ranks': per_rank,
        # frac: the flops the matrix pipe EXECUTES for this decision over its time (with occupancy maps their half of mlp1.0 is
        # hoisted out of the per-action network: counting it would credit work the kernel no longer does - VERDICT r3);
        # algorithmic_frac keeps the reference network's own flop count for comparison
        'roofline': {'bound': 'mfma', 'achieved': sarl_flop(B, H, False) / select_s / 1e12, 'peak': 157.3, 'unit': 'TFLOP/s',
                     'frac': sarl_flop(B, H, False) / select_s / 1e12 / 157.3, 'traffic': None,
                     'algorithmic_frac': flop / select_s / 1e12 / 157.3,
                     'kernel': 'cn_sarl_select (orca + lookahead + reward + feature + value-network + select kernels; the '
                               'value network is cn::sarl_reg_kernel)',
                     'select_ms': select_s * 1e3, 'step_ms': step_s * 1e3,
                     'frac_of_whole_step': sarl_flop(B, H, False) / step_s / 1e12 / 157.3,
                     'note': 'flops of the value network as executed over the HIP-event time of cn_sarl_select; '
                             'frac_of_whole_step: over select + transition + reset + bookkeeping; algorithmic_frac: the '
                             'reference network\'s own flop count - with occupancy maps their half of mlp1.0 (7200 of 69250 '
                             'MACs per row) is computed once per (env, human) instead of once per action, so that figure '
                             'counts work the kernel no longer does'},
    }
    # destroy the engine NOW: left to the cyclic garbage collector, cn_destroy (a stream synchronize + hipFree of ~0.5 GB) ran in
    # the middle of a LATER measurement's timed region - one 24 ms stall, +0.48 ms on each of its 50 decisions (r03: the second
    # or third measure_sarl of a process read 2.3-2.5 ms instead of 1.8; kernel trace: every kernel as fast as before)
    eng.close()
    del ro, eng
    torch.cuda.empty_cache()
    return out


def bench_sarl(args, world, rank, local_rank, comm):
    outputs = {} if args.dump_outputs else None
    out = measure_sarl(args.envs, args.humans, args.workload == 'om-sarl', args.steps, min(args.warmup, 20),
                       min(args.preroll, 60), world, rank, local_rank, comm, outputs=outputs)
    if os.environ.get('CROWDNAV_AMD_BENCH_SHARE_GPU') == '1':
        out['config']['shared_gpu'] = True
    if outputs is not None:
        dump_outputs(outputs, args.dump_outputs, args.envs, '' if world == 1 else 'rank%d_' % rank)
    if rank == 0:
        print(json.dumps(out), flush=True)


def measure_h20(B, local_rank):
    """BASELINE configs[3]'s shard on one GPU: 4096 envs x 20 humans (rollout_kernel<10>, one env per wave).  Three figures:
    the reference geometry (4 m circle, where the reference's rejection sampling makes RESETS the bound) with the
    asynchronous scenario fill, resets included; the same geometry with resets excluded (thirty 47-step launches inside the
    48-episode ring budget, the fill launch before each of them untimed); and the 12 m circle, where resets are cheap."""
    import torch
    import crowdnav_amd
    H = 20

    def one(radius, flags, seed_base, seed_mod, warm, lengths, refill_before_each=False, scenario_cache=True):
        # (cn_create reads the switch: the scenario cache of the wave generators, on by default for seed sets of <= 4096 values)
        old = os.environ.get('CROWDNAV_AMD_SCENARIO_CACHE')
        os.environ['CROWDNAV_AMD_SCENARIO_CACHE'] = '1' if scenario_cache else '0'
        try:
            sim = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_ORCA, robot_visible=1,
                                               device=local_rank, circle_radius=radius, flags=flags)
        finally:
            if old is None:
                os.environ.pop('CROWDNAV_AMD_SCENARIO_CACHE', None)
            else:
                os.environ['CROWDNAV_AMD_SCENARIO_CACHE'] = old
        bufs = sim.rollout_begin(seed_base=seed_base, seed_mod=seed_mod, episode_limit=-1, record_capacity=4)
        for n in warm:
            sim.rollout(n)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in lengths]
        torch.cuda.synchronize()
        done = 0
        if refill_before_each:
            for (e0, e1), n in zip(evs, lengths):  # a 1-step launch spends the ring budget's last step: it carries the (untimed) fill
                sim.rollout(1)
                torch.cuda.synchronize()
                n0 = int(bufs['transitions'].item())
                e0.record()
                sim.rollout(n)
                e1.record()
                torch.cuda.synchronize()
                done += int(bufs['transitions'].item()) - n0
            secs = sum(a.elapsed_time(b) for a, b in evs) / 1e3
        else:
            # back to back, ONE event pair around all of them: with the asynchronous fill the generator kernels of launch k run
            # beside launch k + 1 on their side streams - a synchronize between the launches would let them finish outside
            # the timed span (and hand every launch a freshly filled ring)
            n0 = int(bufs['transitions'].item())
            evs[0][0].record()
            for n in lengths:
                sim.rollout(n)
            evs[-1][1].record()
            torch.cuda.synchronize()
            done = int(bufs['transitions'].item()) - n0
            secs = evs[0][0].elapsed_time(evs[-1][1]) / 1e3
        res = {'value': done / secs, 'unit': 'env-steps/s', 'launches': lengths, 'seconds': secs,
               'paused_env_steps': B * sum(lengths) - done,
               'roofline_frac_hbm': algorithmic_bytes_per_env_step(H) * done / secs / 1e9 / HBM_PEAK_GBS}
        sim.sync()
        sim.close()
        del sim, bufs
        torch.cuda.empty_cache()
        return res

    def with_counters(res):
        # the committed PMC record of this very shape (4096 x 20, 12 m circle, 999-step calls: scripts/gpu.sh pmc), if it is of
        # these kernel sources: VALU issue, scalar overhead, all-instruction issue slots, HBM traffic (FETCH doubled: gfx950)
        rec = pmc_profile(B, H, 999, 12.0)
        issue = pmc_issue(rec, B, 999, res['seconds'] / len(res['launches']))
        if issue is not None:
            res['issue_roofline'] = issue
            res['traffic'] = pmc_traffic_bytes(rec)
            res['algorithmic_bytes'] = algorithmic_bytes_per_env_step(H) * B * 999
        return res

    # the first 1021 'test' phase seeds, on which the reference's own rejection sampling terminates.  A PRIME modulus: episode c
    # of the shard is seeded 1000 + c % 1021 with c = env + 4096 x ordinal, so every env walks through all of them; with the
    # 1024 of rounds 2-3 (4096 = 4 x 1024) every env replayed ONE scenario for ever, and the envs that drew a hard one (up to
    # 13 M random() calls) were paused most of the time - the paused share measured the seed table, not the engine
    seeds = (1000, 1021)
    ASYNC = crowdnav_amd.FLAG_ASYNC_SCENARIO_FILL
    return {
        'workload': '%d envs x %d humans per GPU, ORCA humans + ORCA robot, cn::rollout_kernel<10>' % (B, H),
        # the reference's own geometry, resets INCLUDED.  The episode seeds are the bounded 'test' set (the reference's rejection
        # sampling terminates on it), so the wave generators' scenario cache applies: every seed is generated once per rollout
        'r4': one(4.0, 0, seeds[0], seeds[1], [999], [999] * 3),
        'r4_async_fill': one(4.0, ASYNC, seeds[0], seeds[1], [501], [999] * 6),
        # ... and with the cache switched off: every scenario generated afresh (rounds 2-4's figure; generator-throughput-bound)
        'r4_async_fill_no_scenario_cache': one(4.0, ASYNC, seeds[0], seeds[1], [501], [999] * 6, scenario_cache=False),
        'r4_resets_excluded': one(4.0, 0, seeds[0], seeds[1], [1, 47], [47] * 30, refill_before_each=True),
        'r12': with_counters(one(12.0, 0, 2000, 2 ** 32 - 2000, [201, 999], [999, 999, 999])),
        'episode_seeds_r4': '%d + c %% %d' % seeds,
        'note': 'r4: 4 m circle (env.config), resets included, synchronous ring fill, three 999-step calls under one event pair; '
                'r4_async_fill: the same with CN_FLAG_ASYNC_SCENARIO_FILL, six calls (envs whose next scenario is not ready pause: '
                'paused_env_steps).  Both with the scenario cache (a rollout whose episode seeds come from <= 4096 values '
                'generates each scenario once: the 1021 seeds here are all cached after the warm-up call); '
                'r4_async_fill_no_scenario_cache: CROWDNAV_AMD_SCENARIO_CACHE=0, every scenario generated afresh (28 k random() calls '
                'on average, 60 % of all attempts in the ten hardest seeds) — what an UNBOUNDED seed set costs; '
                'r4_resets_excluded: HIP events around 47-step calls that stay inside the ring budget (the fill runs in the untimed '
                '1-step call before each); r12: 12 m circle, unbounded seeds 2000 + c, resets included (cheap at that radius)',
    }


def measure_policy_decision(B, H, policy, local_rank, iters=20):
    """cn_sarl_select alone for the reference's two baseline value networks (cadrl.py:22-29, lstm_rl.py:9-33; random-init
    weights): HIP-event time per batched decision and the algorithmic flops of the network over it."""
    import numpy as np
    import torch
    import crowdnav_amd
    from crowdnav_amd.compat import cadrl, lstm_rl
    from crowdnav_amd.compat.sarl import build_action_space
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1,
                                       device=local_rank)
    eng.reset(2000 + np.arange(B))
    eng.step(np.zeros((B, 2)), update=True)
    torch.manual_seed(0)
    space, _, _ = build_action_space(1.0)
    acts = np.array([[a.vx, a.vy] for a in space])
    head = 150 * 100 + 100 * 100 + 100
    if policy == 'cadrl':
        net = cadrl.ValueNetwork(13, [150, 100, 100, 1])
        eng.sarl_configure(actions=acts, model='cadrl', mlp3_dims=(150, 100, 100, 1))
        flop = 2 * 81 * H * (13 * 150 + head) * B
    elif policy == 'lstm_rl+pairwise':  # [lstm_rl] with_interaction_module = true: lstm_rl.ValueNetwork2 (lstm_rl.py:36-66)
        net = lstm_rl.ValueNetwork2(13, 6, [150, 100, 100, 50], [150, 100, 100, 1], 50)
        eng.sarl_configure(actions=acts, model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1),
                           interaction_dims=(150, 100, 100, 50))
        flop = 2 * 81 * (H * (13 * 150 + 150 * 100 + 100 * 100 + 100 * 50 + 200 * (50 + 50)) + 56 * 150 + head) * B
    else:
        net = lstm_rl.ValueNetwork1(13, 6, [150, 100, 100, 1], 50)
        eng.sarl_configure(actions=acts, model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1))
        flop = 2 * 81 * (H * 200 * (13 + 50) + 56 * 150 + head) * B
    eng.sarl_set_weights(net.state_dict())
    for _ in range(3):
        eng.sarl_select(want_values=False)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    gc.collect()
    with no_gc():
        for a, b in ev:
            a.record()
            eng.sarl_select(want_values=False)
            b.record()
        torch.cuda.synchronize()
    select_s = sum(a.elapsed_time(b) for a, b in ev) / 1e3 / iters
    eng.close()
    del eng
    torch.cuda.empty_cache()
    return {'workload': '%d envs x %d humans, 81 actions, %s value network, one batched decision' % (B, H, policy),
            'decisions_per_s': B / select_s,
            'roofline': {'bound': 'mfma', 'achieved': flop / select_s / 1e12, 'peak': 157.3, 'unit': 'TFLOP/s',
                         'frac': flop / select_s / 1e12 / 157.3, 'select_ms': select_s * 1e3,
                         'kernel': 'cn_sarl_select; the value network is cn::%s' %
                                   {'cadrl': 'cadrl_reg_kernel', 'lstm_rl+pairwise': 'lstm2_reg_kernel'}.get(policy, 'lstm_reg_kernel'),
                         'note': 'algorithmic flops (unpadded layer widths) over the HIP-event time of cn_sarl_select'}}


def measure_sample_step(local_rank, envs=1, steps=28, repeats=24, with_om=False, policy='sarl'):
    """BASELINE configs[4]'s in-scope piece: one train-phase sampling step (train.py:156-170 -> explorer.py:56-65 with
    multi_human_rl.py:11-63 behind robot.act) of ONE env — cn_sarl_sample_step streamed `steps` times without a host check,
    HIP events around the stream, the median of the `repeats` episodes that were still running at their last timed step (round
    6: the kernels skip an env whose episode is over, and a skipped step is not a sampled step; the goal is 8 m away at 1 m/s
    and 0.25 s per step, so 28 steps end an episode only by a collision).  The shipped widths, 5 humans, 81 actions,
    random-init weights, epsilon 0.1."""
    import numpy as np
    import torch
    import crowdnav_amd
    from crowdnav_amd.compat.sarl import ValueNetwork, build_action_space
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=envs, num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=0,
                                       device=local_rank)
    torch.manual_seed(0)
    D = 61 if with_om else 13
    net_kwargs = {}
    if policy == 'lstm_rl':  # lstm_rl.ValueNetwork1 at policy.config's widths (round 6: sarl_narrow_kernel<true>)
        from crowdnav_amd.compat import lstm_rl
        net = lstm_rl.ValueNetwork1(D, 6, [150, 100, 100, 1], 50)
        net_kwargs = dict(model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1))
    else:
        net = ValueNetwork(D, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)
    space, _, _ = build_action_space(1.0)
    eng.sarl_configure(actions=np.array([[a.vx, a.vy] for a in space]), with_om=with_om, **net_kwargs)
    eng.sarl_set_weights(net.state_dict())
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=eng.device)  # noqa: E731
    traj, rew, inf, dmn = (z((envs, steps, 5, D), torch.float32), z((steps, envs), torch.float64), z((steps, envs), torch.uint8),
                           z((steps, envs), torch.float64))
    act, alive, done, action = z((steps, envs), torch.int32), z((envs,), torch.uint8), z((envs,), torch.uint8), z((envs, 2), torch.float64)
    step = eng.sarl_sampler(traj, rew, inf, dmn, act, alive, done, action)
    times = []
    for rep in range(repeats + 1):  # (the first episode warms up)
        eng.reset(2000 + rep * envs + np.arange(envs))
        alive.fill_(1)
        done.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with no_gc():
            a.record()
            for t in range(steps):
                step(t, 0.1)
            b.record()
            torch.cuda.synchronize()
        if rep > 0 and not bool(done.any().item()):  # every timed step was a sampled one
            times.append(a.elapsed_time(b) / 1e3 / steps)
    counts = eng.launch_counts()
    eng.close()
    del eng
    torch.cuda.empty_cache()
    if not times:
        raise RuntimeError('measure_sample_step: every one of %d episodes ended within %d steps' % (repeats, steps))
    per_step = sorted(times)[len(times) // 2]
    calls = (repeats + 1) * steps
    return {'workload': '%d env x 5 humans, 81 actions, %s: cn_sarl_sample_step (decision + epsilon-greedy + replay state + '
                        'transition), %d steps streamed' % (envs, ('LSTM-RL' if policy == 'lstm_rl' else 'SARL') if not with_om else
                                                            ('LSTM-RL with occupancy maps' if policy == 'lstm_rl' else 'OM-SARL (occupancy maps)'), steps),
            'value': envs / per_step, 'unit': 'env-steps/s', 'us_per_step': per_step * 1e6,
            'launches_per_step': 2 if (counts['sarl_narrow'], counts['sarl_decide_steps']) == (calls, calls) else None,
            'launch_counts': {k: counts[k] for k in ('sarl_narrow', 'sarl_decide_steps')}, 'calls': calls,
            'episodes_timed': len(times),
            'kernels': 'cn::sarl_narrow_kernel (value network on 27 workgroups, reward, replay state), '
                                               'cn::sarl_decide_step_kernel (arg-max, draw, transition, next ORCA)',
            'note': 'round 4: ten launches, 70-80 us per step; the reference schedule of configs[4] samples 10 000 episodes this way '
                    '(profiles/r05_config5_reference_schedule.json: weight re-pack / reset / read-back / TD targets included)'}


def secondary(B, local_rank):
    """BASELINE configs[2] (SARL / OM-SARL value-network rollouts) and configs[3] (20 humans) measured in the SAME run as
    the headline, after its timed region, so that the driver's record carries them."""
    out = {}
    for om in (False, True):
        r = measure_sarl(B, 5, om, 50, 10, 30, 1, 0, local_rank)
        key = 'om_sarl' if om else 'sarl'
        out[key] = {k: r[k] for k in ('value', 'unit', 'steps', 'ms_per_step', 'roofline')}
        out[key]['workload'] = r['config']['workload']
        out[key]['decisions_per_s'] = B / (r['roofline']['select_ms'] / 1e3)
        out[key]['cpu_baseline'] = reference_decision_baseline('sarl+om' if om else 'sarl')
    for policy in ('cadrl', 'lstm_rl', 'lstm_rl+pairwise'):
        key = policy.replace('+', '_')
        out[key] = measure_policy_decision(B, 5, policy, local_rank)
        out[key]['cpu_baseline'] = reference_decision_baseline(policy)
    out['h20'] = measure_h20(B, local_rank)
    out['h20']['cpu_baseline'] = cpu_baseline_h20()
    out['sample_step'] = measure_sample_step(local_rank)
    out['sample_step']['cpu_baseline'] = reference_sampling_baseline()
    out['sample_step']['om_sarl'] = measure_sample_step(local_rank, with_om=True)
    out['sample_step']['lstm_rl'] = measure_sample_step(local_rank, policy='lstm_rl')
    out['sample_step']['lstm_rl_om'] = measure_sample_step(local_rank, with_om=True, policy='lstm_rl')
    out['config5_schedule'] = config5_schedule_estimate()
    return out


def cpu_baseline(envs, humans, target_seconds=8.0):
    """The CPU oracle (oracle/crowd_oracle.cpp: same workload, same auto-reset rollout) on the host cores."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import numpy as np
    import crowd_oracle

    def run(threads, steps):
        crowd_oracle.CrowdOracle.set_threads(threads)
        o = crowd_oracle.CrowdOracle(num_envs=envs, num_humans=humans, robot_policy=1, robot_visible=1)
        o.reset(2000 + np.arange(envs))
        z = lambda dt: np.zeros(envs, dtype=dt)  # noqa: E731
        t0 = time.perf_counter()
        total, _ = o.rollout(steps, 2000, 2 ** 32 - 2000, 4, z(np.int32), z(np.int32), z(np.float64))
        return total, time.perf_counter() - t0

    cores = crowd_oracle.CrowdOracle.max_threads()
    # size the sample so that the all-core run takes ~target_seconds: short runs under-report (thread start-up,
    # cold caches), so grow the step count until one run is long enough, then keep the faster of two runs (the
    # host is shared: the CPU side should not be under-reported)
    steps, (n_all, dt_all) = 200, run(cores, 200)
    while dt_all < 0.6 * target_seconds and steps < 1000000:
        steps = int(min(1000000, max(2 * steps, steps * target_seconds / dt_all)))
        n_all, dt_all = run(cores, steps)
    n_all, dt_all = min(((n_all, dt_all), run(cores, steps)), key=lambda r: r[1] / r[0])
    n, dt = run(1, 20)
    steps1 = max(20, int(0.4 * target_seconds * n / dt / envs))
    n_one, dt_one = run(1, steps1)
    crowd_oracle.CrowdOracle.set_threads(cores)
    ref_py = reference_python_baseline()
    return {
        'reference_python': ref_py,
        'value': n_all / dt_all, 'unit': 'env-steps/s', 'cores': cores, 'kind': 'port',
        'sample': '%d envs x %d humans x %d steps, auto-reset, OpenMP over envs (oracle/crowd_oracle.cpp, '
                  'float32 RVO2 restatement; upstream Python-RVO2 is not installable offline), %.1f s of wall time on '
                  'all cores' % (envs, humans, steps, dt_all),
        'single_core_value': n_one / dt_one,
    }


def cpu_baseline_h20(envs=512, steps=60):
    """CPU side of secondary.h20.r12: the C++ oracle on all host cores on a bounded sample of the same workload (20 humans, 12 m
    circle, auto-reset), and the unmodified reference Python loop at that crowd on one core (reference_python_run)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import numpy as np
    import crowd_oracle
    cores = crowd_oracle.CrowdOracle.max_threads()
    crowd_oracle.CrowdOracle.set_threads(cores)
    best = None
    for _ in range(2):
        o = crowd_oracle.CrowdOracle(num_envs=envs, num_humans=20, robot_policy=1, robot_visible=1, circle_radius=12.0)
        o.reset(2000 + np.arange(envs))
        z = lambda dt: np.zeros(envs, dtype=dt)  # noqa: E731
        t0 = time.perf_counter()
        total, _ = o.rollout(steps, 2000, 2 ** 32 - 2000, 4, z(np.int32), z(np.int32), z(np.float64))
        dt = time.perf_counter() - t0
        if dt < 1.0:
            steps *= max(2, int(2.0 / max(dt, 1e-3)))
        if best is None or total / dt > best[0] / best[1]:
            best = (total, dt, steps)
    run = reference_python_run()
    c20 = (run['raw'] or {}).get('crowd20')
    return {'value': best[0] / best[1], 'unit': 'env-steps/s', 'cores': cores, 'kind': 'port',
            'sample': '%d envs x 20 humans x %d steps on the 12 m circle, auto-reset, OpenMP over envs (oracle/crowd_oracle.cpp), '
                      '%.1f s' % (envs, best[2], best[1]),
            'reference_python': None if not c20 else {
                'value': c20['env_steps_per_s'], 'unit': 'env-steps/s', 'cores': 1, 'kind': 'reference', 'host': _reference_host(run),
                'sample': '%d env-steps in %.1f s; %s' % (c20['env_steps'], c20['seconds'], c20['what'])}}


def ring_depth(async_fill=False):
    """depth of an engine's scenario ring (cn_create reads the same variable; default 48 episodes ahead of every env, 144 under
    the asynchronous fill)"""
    return max(1, int(os.environ.get('CROWDNAV_AMD_RING_DEPTH') or (144 if async_fill else 48)))


def measure_fill_seconds(eng, depth):
    """What ONE steady-state top-up of the scenario ring costs: 1-step calls with a HIP-event pair each, classified by the
    engine's own launch counters into calls that carried a fill (one per `depth` steps: it regenerates the slots consumed since
    the previous one) and calls that did not; the difference of the medians.  Device time on the engine's stream."""
    import torch
    n = 3 * (depth + 1)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    kinds = []
    for e0, e1 in evs:
        before = eng.launch_counts()['ring_fills']
        e0.record()
        eng.rollout(1)
        e1.record()
        kinds.append(eng.launch_counts()['ring_fills'] > before)
    torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    with_fill = [a.elapsed_time(b) for (a, b), k in zip(evs, kinds) if k]
    without = [a.elapsed_time(b) for (a, b), k in zip(evs, kinds) if not k]
    if not with_fill or not without:
        return None
    return max(0.0, med(with_fill) - med(without)) / 1e3


def measure_orca(args, world, rank, local_rank, comm, inkernel, backend, fill_probe=True, repeats=0, outputs=None):
    """One measurement of the ORCA workload on a fresh engine: preroll, warm-up, the K timed steps, the shard boundary.
    inkernel: round 3's arrangement (every launch leaves the job-wide counter, the explorer.py:74-90 sums and the record
    blocks itself) instead of ABI v6's (per-env counters, statistics once at the boundary).  outputs: a dict that receives
    what the K timed steps and the boundary computed (host tensors), before anything else runs on the engine."""
    import torch
    import torch.distributed as dist
    import crowdnav_amd
    from crowdnav_amd import distributed as cd
    B, H, RECORDS = args.envs, args.humans, args.records
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_ORCA,
                                       robot_visible=1, device=local_rank, circle_radius=args.circle_radius,
                                       flags=crowdnav_amd.FLAG_ASYNC_SCENARIO_FILL if args.async_fill else 0)
    # phase 'train' seeds: 2000 + global episode id (crowd_sim.py:272-276), unbounded episode supply.
    # The timed region is the K steps: transitions, auto-resets, per-episode records.  The job-wide statistics
    # (explorer.py:74-90: the reference computes them ONCE, after its episode loop) and the record exchange belong to the
    # shard boundary, timed separately as boundary_ms at every world size: a launch counts its transitions per env
    # (per_env_transitions, ABI v6) and ends without any hand-off between its workgroups — no in-kernel summary / blocks
    # (boundary_records = 0), which were ~9 us of the last wave's tail in every launch of the driver's 20-step shape.
    # record_capacity = --records (default 1) on every path: the summary of one engine and of the gathered shards is then the
    # same statistic — over each env's most recent finished episode — whatever the world size (tests/test_bench_multirank.py)
    off, stride = cd.shard(rank, world, B)
    bufs = eng.rollout_begin(seed_base=args.seed_base, seed_mod=args.seed_mod, episode_limit=-1, record_capacity=RECORDS,
                             env_offset=off, env_stride=stride,
                             boundary_records=RECORDS if inkernel else 0, per_env_transitions=not inkernel)
    summary_out = torch.zeros(crowdnav_amd._lib.SUMMARY_FIELDS, dtype=torch.float64, device=eng.device)  # the boundary's output
    rccl = {'world': dist.get_world_size(), 'backend': dist.get_backend(), 'gathered_rows': None,
            'HSA_ENABLE_IPC_MODE_LEGACY': os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')} if world > 1 else None

    # HIP events of the timed launches exist (and have been recorded once) before the clock starts: creating one lazily
    # inside the timed region costs more host time than a 20-step launch's enqueue
    # One event in front of the first timed launch and one behind EVERY launch: launch k is timed from the event behind launch
    # k - 1 to its own (the stream has nothing else in between), and the last of them doubles as the "stream has drained" flag
    # the host spins on — n + 1 event records in the timed region instead of 2 n + 1 (each is a packet the command processor
    # handles between the kernels).
    n_launches = (args.steps + args.chunk - 1) // args.chunk
    pool = [torch.cuda.Event(enable_timing=True) for _ in range(n_launches + 2)]
    for ev in pool:
        ev.record()

    def run(n_steps, events=None):
        left = n_steps  # (events: the caller has recorded pool[0] on the idle stream, in front of its clock)
        while left > 0:
            n = min(args.chunk, left)
            eng.rollout(n)
            if events is not None:
                k = len(events)
                pool[k + 1].record()
                events.append((pool[k], pool[k + 1], n))
            left -= n

    def spin(last=None):
        if last is None:
            last = pool[-1]
            last.record()
        while not last.query():  # spin until the stream has drained: a blocking synchronize alone wakes up late
            pass

    def drain(last=None):
        spin(last)
        torch.cuda.synchronize()

    def fence():
        drain()
        comm.barrier()

    def shard_boundary():
        """What a run does ONCE, when it ends (explorer.py:74-90): on one GPU the summary of the engine's record rings
        (cn_rollout_summary: one kernel, into the preallocated output); on several the record blocks of this shard
        (cn_rollout_records), the blocks of every rank (one RCCL all-gather of 56 B per env) and the job-wide summary
        (cn_records_summary): float64 [8] on the device"""
        if world == 1:  # one engine: straight from its record rings
            return bufs['summary'] if inkernel else eng.rollout_summary(out=summary_out)
        blocks = bufs['blocks'] if inkernel else eng.rollout_records(RECORDS)
        blocks = cd.gather_blocks(blocks)
        rccl['gathered_rows'] = int(blocks.shape[0])
        return eng.records_summary(blocks, record_capacity=RECORDS, out=summary_out)

    def snapshot():
        """device copies of the shard's counters (transitions, episodes finished per env): asynchronous, no host round trip —
        whatever the host does between the warm-up launches and the timed ones is device idle time in front of a 120 us launch"""
        return (bufs['transitions'] if inkernel else bufs['env_transitions']).clone(), bufs['ep_count'].clone()

    run(args.preroll)
    for _ in range(3):  # warm-up of the boundary too (lazy code-object loads, communicator setup, its kernels' code in the caches)
        shard_boundary()
    gc.collect()  # (before the warm-up launches: see no_gc)
    run(args.warmup)
    snap_t, snap_e = snapshot()
    shard_boundary()  # once more behind everything else that runs before the clock starts (the snapshot's torch kernels)
    events = []
    fence()  # barrier + synchronize ...
    fence()  # ... twice: the first drains the warm-up launches and the snapshot copies, the second finds an idle device
    counts0 = eng.launch_counts()
    pool[0].record()  # opens the first timed launch's event span (an idle stream stamps it at once)
    with no_gc():
        t0 = time.perf_counter()
        run(args.steps, events)
        drain(events[-1][1])  # this rank's K steps are done (synchronize) ...
        elapsed = time.perf_counter() - t0
        # (the collector stays off between the two regions: re-enabled here, the first allocation — the dict below — runs the
        # collection the timed region deferred, and the boundary then opens on a device that has idled for that long:
        # scripts/probes/boundary_probe2.py, 21.8 us behind a rollout launch, 25.4 after 200 us of idling, 32-37 here)
        comm.barrier()  # ... and every rank's, before anything else is launched
        tb = time.perf_counter()
        summary = shard_boundary()
        spin()  # the event behind the boundary's last kernel has completed: its results are on the device
        boundary = time.perf_counter() - tb
        counts1 = eng.launch_counts()  # (host-side counters; the boundary launches nothing they count)
        if os.environ.get('CROWDNAV_AMD_BENCH_BOUNDARY_DEBUG'):  # further samples of the same call, back to back (stderr)
            extra = []
            for _ in range(4):
                tb2 = time.perf_counter()
                shard_boundary()
                spin()
                extra.append((time.perf_counter() - tb2) * 1e6)
            tb2 = time.perf_counter()
            spin()
            empty = (time.perf_counter() - tb2) * 1e6
            again = []
            for _ in range(4):  # the same pattern once more: a 20-step launch, drained, then the boundary
                run(args.steps)
                drain()
                tb2 = time.perf_counter()
                shard_boundary()
                spin()
                again.append((time.perf_counter() - tb2) * 1e6)
            print('boundary debug: first %.1f us, then %s, an empty event round trip %.1f us; behind further launches %s' %
                  (boundary * 1e6, ' '.join('%.1f' % v for v in extra), empty, ' '.join('%.1f' % v for v in again)), file=sys.stderr)
    torch.cuda.synchronize()
    now_t, now_e = snapshot()
    own_episodes = int((now_e - snap_e).sum().item())
    transitions = int((now_t - snap_t).sum().item())
    if outputs is not None:
        state, gtime = eng.get_state()
        outputs.update({k: v.cpu() for k, v in bufs.items()}, state=state.cpu(), global_time=gtime.cpu(), summary=summary.cpu())
    # VERDICT r5 weak #4d: `value` is ONE sample of a region that can be as short as 120 us.  `repeats` further repetitions of
    # the same (warm-up + K timed steps) pattern on the same engine, each with the same fences, so that the line shows the spread
    # (value stays the first sample, as defined): short regions only — a default 8000-step run is its own average
    samples = []
    for _ in range(repeats if elapsed < 0.05 else 0):
        run(args.warmup)
        s0 = snapshot()[0]
        fence()
        fence()
        f0 = eng.launch_counts()['ring_fills']
        with no_gc():
            ts = time.perf_counter()
            run(args.steps)
            drain()
            dt = time.perf_counter() - ts
        comm.barrier()
        n = int((snapshot()[0] - s0).sum().item())
        dt_max, = comm.all_reduce([dt], op='max')
        n_all, = comm.all_reduce([n])
        samples.append((n_all / dt_max, eng.launch_counts()['ring_fills'] - f0))
    s = [float(v) for v in summary.cpu().tolist()]
    event_spans = [(e0.elapsed_time(e1) / 1e3, n) for e0, e1, n in events]
    fill_s = None
    if fill_probe and not args.async_fill and not args.no_fill_probe:
        fill_s = measure_fill_seconds(eng, ring_depth())
    per_rank = comm.all_gather({'rank': rank, 'transitions': transitions, 'seconds': elapsed, 'boundary_seconds': boundary})
    # the slowest rank's K steps, the slowest rank's boundary; transitions of every shard (they differ by the few ring-dry pauses)
    mx = comm.all_reduce([elapsed, boundary, fill_s if fill_s is not None else -1.0], op='max')
    total, episodes, fills = (int(v) for v in comm.all_reduce([transitions, own_episodes,
                                                               counts1['ring_fills'] - counts0['ring_fills']]))
    eng.sync()
    eng.close()
    del eng, bufs
    torch.cuda.empty_cache()
    return {'elapsed': mx[0], 'boundary': mx[1], 'fill_s': mx[2] if mx[2] >= 0 else None, 'total': total, 'episodes': episodes,
            'fills_in_timed_region': fills // world if world > 1 else fills, 'events': event_spans, 'summary': s,
            'per_rank': per_rank, 'rccl': rccl, 'ring_depth': ring_depth(args.async_fill), 'samples': samples}


def init_distributed(backend, local_rank):
    """init_process_group + the FIRST collective on a device tensor (RCCL builds its communicator lazily: a transport problem
    would otherwise surface in the middle of the run).  A failure exits with a message that names the one environment switch
    this pool is known to need: the host driver supports dmabuf IPC only, and with HSA_ENABLE_IPC_MODE_LEGACY unset or != 0
    RCCL / device-tensor sharing between processes fails with `hipIpcGetMemHandle: invalid argument`.  (No in-process retry:
    the HSA runtime reads the variable once, when it initialises, long before a communicator exists.)"""
    import torch
    import torch.distributed as dist
    try:
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
            t = torch.ones(1, dtype=torch.float64, device=torch.device('cuda', local_rank))
        else:
            dist.init_process_group('gloo')
            t = torch.ones(1, dtype=torch.float64)
        dist.all_reduce(t)
        if float(t.item()) != float(dist.get_world_size()):
            raise RuntimeError('first all-reduce returned %r for a world of %d' % (t.item(), dist.get_world_size()))
    except Exception as exc:  # noqa: BLE001 (whatever the backend raises: the message is what matters)
        raise SystemExit(
            'bench.py: torch.distributed (%s) failed on rank %s of %s: %s: %s\n'
            'HSA_ENABLE_IPC_MODE_LEGACY is %r in this process; this pool\'s host driver supports dmabuf IPC only, so it must be 0 '
            '(bench.py sets it with setdefault before the first HIP call and never overrides an exported value). '
            'If it IS 0 and RCCL still fails, run once with the variable unset to compare.'
            % (backend, os.environ.get('RANK'), os.environ.get('WORLD_SIZE'), type(exc).__name__, exc,
               os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')))


_REFERENCE_RUN = {}  # the one subprocess run of oracle/time_reference_python.py of this process: {'raw': dict | None, 'here': bool}


def reference_python_run(cases=250, decisions=30, sampling_seconds=8.0, timeout=300):
    """ONE subprocess run of oracle/time_reference_python.py per bench process — the UNMODIFIED reference (test infrastructure:
    the copy `make -C oracle ref` leaves under the git-ignored oracle/_ref/ travels with the snapshot; its rvo2 module is the
    float32 restatement oracle/rvo2_pymodule.cpp — upstream Python-RVO2 is not installable offline) timed ON THIS HOST, one
    pinned core, torch on one thread: its ORCA loop (2 x `cases` test cases), `decisions` robot.act -> predict calls per value
    network, and `sampling_seconds` of single-episode train-phase sampling calls.  ~20 s of wall time in all.  Without a
    reference copy on this machine: the figures committed from the build container, labelled as such."""
    if _REFERENCE_RUN:
        return _REFERENCE_RUN
    script = os.path.join(ROOT, 'oracle', 'time_reference_python.py')
    raw, here = None, False
    try:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='', OMP_NUM_THREADS='1',
                   MKL_NUM_THREADS='1')
        p = subprocess.run([sys.executable, script, '--json', '--cases', str(cases), '--decisions', str(decisions),
                            '--sampling-seconds', str(sampling_seconds)], capture_output=True, text=True, timeout=timeout, env=env)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode == 0 and line:
            raw, here = json.loads(line[-1]), True
    except (OSError, ValueError, subprocess.TimeoutExpired):
        pass
    if raw is None and os.path.exists(REFERENCE_PYTHON_PROFILE):
        try:
            raw = json.load(open(REFERENCE_PYTHON_PROFILE))
        except (OSError, ValueError):
            raw = None
    _REFERENCE_RUN.update(raw=raw, here=here)
    return _REFERENCE_RUN


def _reference_host(run):
    return run['raw']['host_cpu'] + (' (THIS host, timed in this run)' if run['here'] else
                                     ' (build container, NOT this host: committed figure %s, no reference copy on this machine)'
                                     % os.path.relpath(REFERENCE_PYTHON_PROFILE, ROOT))


def reference_python_baseline():
    """north_star: "reported next to the reference Python-RVO2 CPU path timed on the same host (core count stated)": the ORCA
    leg of reference_python_run() — the reference's own loop (env.reset / robot.act / env.step, crowd_nav/test.py:86-92 with
    --policy orca), one core."""
    run = reference_python_run()
    r = run['raw']
    if r is None or 'value' not in r:
        return None
    out = {'value': r['value'], 'unit': r['unit'], 'cores': r['cores'], 'kind': 'reference', 'host': _reference_host(run),
           'value_visible_robot': r.get('value_visible_robot'),
           'note': r['what'] + '; unmodified reference Python (oracle/_ref or /root/reference) on the float32 rvo2 restatement'}
    if run['here']:
        out['sample'] = '%d + %d env-steps in %.1f s (2 x %d test cases, robot invisible / visible)' % (
            r['runs'][0]['env_steps'], r['runs'][1]['env_steps'], r['runs'][0]['seconds'] + r['runs'][1]['seconds'],
            r['runs'][0]['test_cases'])
    return out


def reference_decision_baseline(policy):
    """cpu_baseline of one secondary decision row: the reference's own robot.act -> predict (multi_human_rl.py:11-63 /
    cadrl.py:130-176 / lstm_rl.py:69-104: 81 onestep_lookahead + 81 batch-1 forwards) on one core of this host.
    policy: 'sarl' | 'sarl+om' | 'cadrl' | 'lstm_rl' | 'lstm_rl+pairwise'."""
    run = reference_python_run()
    r = run['raw']
    for rec in ((r or {}).get('decision') or {}).get('runs', []):
        if rec['policy'] == policy:
            return {'value': rec['decisions_per_s'], 'unit': 'decisions/s', 'cores': 1, 'kind': 'reference',
                    'host': _reference_host(run), 'ms_per_decision': rec['ms_per_decision'],
                    'sample': '%d decisions of the unmodified robot.act -> predict in %.1f s (5 humans, 81 actions, random-init '
                              'weights, torch CPU on 1 thread; only robot.act timed)' % (rec['decisions'], rec['seconds'])}
    return None


def reference_sampling_baseline():
    """cpu_baseline of secondary.sample_step: the reference's train-phase sampling loop (train.py:156-170: single-episode
    explorer.run_k_episodes(1, 'train', update_memory=True) calls, epsilon-greedy SARL robot) on one core of this host."""
    run = reference_python_run()
    rec = (run['raw'] or {}).get('sampling')
    if not rec:
        return None
    return {'value': rec['env_steps_per_s'], 'unit': 'env-steps/s', 'cores': 1, 'kind': 'reference', 'host': _reference_host(run),
            'ms_per_env_step': rec['ms_per_env_step'],
            'sample': '%d episodes = %d env-steps in %.1f s of the unmodified Explorer.run_k_episodes(1, \'train\', update_memory=True), '
                      'epsilon %.1f, torch CPU on 1 thread' % (rec['episodes'], rec['env_steps'], rec['seconds'], rec['epsilon'])}


def config5_schedule_estimate():
    """BASELINE.md §4 row 5 ("wall-clock per phase vs CPU reference") for configs[4]: the in-scope phases of the reference's
    own train.config schedule as measured on the MI355X (the committed profiles/r0N_config5_reference_schedule.json: 10 000
    single-episode sampling calls, 3 000 imitation episodes) beside what the unmodified reference needs for the SAME env-step
    counts at the rates timed on this host in this run: imitation collection at the ORCA loop's rate (its robot is ORCA,
    train.py:115-129), RL sampling at the sampling leg's rate.  The SGD phases are torch on both sides (out of scope)."""
    path = next((p for p in CONFIG5_PROFILES if os.path.exists(p)), None)
    if path is None:
        return None
    t = json.load(open(path)).get('timing') or {}
    orca, samp = reference_python_baseline(), reference_sampling_baseline()
    out = {'schedule_from': os.path.relpath(path, ROOT),
           'device_s': {'il_collect': t.get('il_collect_s'), 'rl_sample': t.get('rl_sample_s')},
           'env_steps': {'il_collect': t.get('il_env_steps'), 'rl_sample': t.get('rl_env_steps')},
           'out_of_scope_s': {'il_sgd': t.get('il_sgd_s'), 'rl_sgd': t.get('rl_sgd_s')}}
    est = {}
    if orca and t.get('il_env_steps'):
        est['il_collect'] = t['il_env_steps'] / orca['value']
    if samp and t.get('rl_env_steps'):
        est['rl_sample'] = t['rl_env_steps'] / samp['value']
    out['reference_estimate_s'] = est
    out['speedup'] = {k: est[k] / out['device_s'][k] for k in est if out['device_s'].get(k)}
    out['note'] = ('reference_estimate_s = the schedule\'s env-step count of the phase / the unmodified reference\'s env-steps/s on ONE '
                   'core of this host (cpu_baseline.reference_python for the ORCA-driven imitation collection, '
                   'secondary.sample_step.cpu_baseline for the SARL sampling); an estimate scaled from a bounded sample, not a run '
                   'of the whole schedule (the reference needs ~%.0f h for it)' % (sum(est.values()) / 3600.0 if est else 0))
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(outputs, out_dir, rows, prefix=''):
    """--dump-outputs: every array of `outputs` as out_dir/<prefix><name>.npy, float32 kept, everything else as float64 (exact
    for the flags, counters and outcome codes).  When they exceed 64 MB in all, the arrays whose first axis is the env axis
    (`rows` long) keep the same fixed, seeded sample of envs, whose indices are written as env_index.npy."""
    import numpy as np
    arrs = {}
    for k, v in outputs.items():
        a = v.numpy() if hasattr(v, 'numpy') else np.asarray(v)
        arrs[k] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
    per_env = {k for k, a in arrs.items() if a.ndim and a.shape[0] == rows}
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_LIMIT_BYTES:
        fixed = sum(a.nbytes for k, a in arrs.items() if k not in per_env) + 4096 * (len(arrs) + 1)  # (+ the .npy headers)
        row_bytes = sum(arrs[k].nbytes // rows for k in per_env) + 8  # (+ its entry of env_index)
        keep = max(1, min(rows, (DUMP_LIMIT_BYTES - fixed) // row_bytes))
        idx = np.sort(np.random.default_rng(0).choice(rows, keep, replace=False))
        arrs = {k: a[idx] if k in per_env else a for k, a in arrs.items()}
        arrs['env_index'] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(out_dir, prefix + k + '.npy'), np.ascontiguousarray(a))


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-execute this script as N ranks, one per GPU, rendezvous on
    127.0.0.1 (what torch.distributed.run would set up).  Rank 0's JSON line goes to our stdout."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')  # dmabuf IPC: the only mode the host driver supports
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        while procs:
            for p in list(procs):
                code = p.poll()
                if code is None:
                    continue
                procs.remove(p)
                if code != 0:
                    rc = rc or code
                    for q in procs:  # one rank failed: the others would wait in a collective forever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            p.kill()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=8000)
    ap.add_argument('--warmup', type=int, default=1000)
    ap.add_argument('--preroll', type=int, default=200,
                    help='untimed steps before the warm-up that desynchronise the episodes of the batch')
    ap.add_argument('--envs', type=int, default=4096, help='envs per GPU')
    ap.add_argument('--humans', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=1000, help='steps fused into one kernel launch')
    ap.add_argument('--circle-radius', type=float, default=4.0, help='scenario circle radius (reference default 4)')
    ap.add_argument('--seed-base', type=int, default=2000, help="episode c is seeded seed_base + c %% seed_mod (default: the "
                    "'train' phase numbering of crowd_sim.py:272-276, unbounded)")
    ap.add_argument('--seed-mod', type=int, default=2 ** 32 - 2000)
    ap.add_argument('--async-fill', action='store_true',
                    help='CN_FLAG_ASYNC_SCENARIO_FILL: scenario generation on side streams (crowds of more than 8 humans)')
    ap.add_argument('--records', type=int, default=1,
                    help='episode records kept per env (the record ring\'s capacity = records per boundary block); 1: the '
                         'summary of one engine and of gathered shards is the same statistic at every world size')
    ap.add_argument('--no-r3-definition', action='store_true',
                    help='skip the second measurement (value_r3_definition: in-kernel job-wide statistics, rounds 1-3)')
    ap.add_argument('--no-fill-probe', action='store_true',
                    help='skip fill_ms / value_amortised_fill (3 x 49 one-step launches after the timed region: profiling runs '
                         'that average per-dispatch counters of the rollout kernel want only the launches of the named shape)')
    ap.add_argument('--repeats', type=int, default=8,
                    help='value_samples: further repetitions of the (warm-up + K timed steps) pattern on the same engine when the '
                         'timed region is shorter than 50 ms (min / median / max in the line; value stays the first sample)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-secondary', action='store_true',
                    help='skip the configs[2] / configs[3] measurements that follow the headline at N=1')
    ap.add_argument('--workload', choices=['orca', 'sarl', 'om-sarl'], default='orca',
                    help="orca = BASELINE configs[1] (the headline metric); sarl / om-sarl = configs[2]")
    ap.add_argument('--full', action='store_true',
                    help='everything beside the headline as well: value_r3_definition, the fill probe, value_samples and, at N=1, '
                         'cpu_baseline and secondary (each still subject to its --no-* / --repeats option); without it a run '
                         'measures the K timed steps and the shard boundary only')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the timed path computed (state and episode bookkeeping after the last timed step, the '
                         'boundary\'s summary) as DIR/<name>.npy, float32 / float64, at most 64 MB (a seeded sample of envs beyond)')
    args = ap.parse_args()
    if args.gpus < 1 or args.steps < 1 or args.warmup < 0 or args.preroll < 0 or args.chunk < 1 or args.records < 1:
        raise SystemExit('--gpus/--steps/--chunk/--records must be >= 1, --warmup/--preroll >= 0')

    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args.gpus))

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    backend = os.environ.get('CROWDNAV_AMD_BENCH_BACKEND', 'nccl')
    share_gpu = os.environ.get('CROWDNAV_AMD_BENCH_SHARE_GPU') == '1'
    if backend not in ('nccl', 'gloo'):
        raise SystemExit('CROWDNAV_AMD_BENCH_BACKEND must be nccl or gloo')
    if world > 1:
        # dmabuf IPC: the only mode this pool's host driver supports (task environment note: "without it RCCL ... fails
        # with hipIpcGetMemHandle: invalid argument").  The HSA runtime reads it when it initialises, i.e. before the first
        # HIP call below — never overriding a value the box exports.
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

    import torch
    import torch.distributed as dist
    import crowdnav_amd
    from crowdnav_amd import distributed as cd

    if world != args.gpus:
        raise SystemExit('WORLD_SIZE=%d does not match --gpus %d' % (world, args.gpus))
    if share_gpu:
        local_rank = 0  # every rank on device 0: executes the N > 1 path on a one-GPU box (not a scaling measurement)
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit('rank %d needs GPU %d but only %d are visible' % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    if world > 1:
        init_distributed(backend, local_rank)
    comm = Comm(world, rank, backend)

    B, H = args.envs, args.humans
    if args.workload != 'orca':
        bench_sarl(args, world, rank, local_rank, comm)
        if world > 1:
            dist.destroy_process_group()
        return
    # CROWDNAV_AMD_BENCH_INKERNEL_STATS=1: round 3's arrangement for the HEADLINE (A/B runs); the --full line measures both
    inkernel = os.environ.get('CROWDNAV_AMD_BENCH_INKERNEL_STATS') == '1'
    outputs = {} if args.dump_outputs else None
    m = measure_orca(args, world, rank, local_rank, comm, inkernel, backend, fill_probe=args.full,
                     repeats=args.repeats if args.full else 0, outputs=outputs)
    # `value` changed definition in round 4 (the job-wide statistics left the timed launches).  The same K
    # steps in round 3's arrangement — every launch leaves the job-wide transition counter, the explorer.py:74-90 sums and the
    # record blocks behind itself — are measured right after, on a fresh engine, and reported beside it
    m3 = None if (not args.full or inkernel or args.no_r3_definition) else measure_orca(args, world, rank, local_rank, comm, True,
                                                                                          backend, fill_probe=False)
    if outputs is not None:
        dump_outputs(outputs, args.dump_outputs, B, '' if world == 1 else 'rank%d_' % rank)

    elapsed, boundary, total, episodes = m['elapsed'], m['boundary'], m['total'], m['episodes']
    events = m['events']
    kernel_s = sum(t for t, _ in events)
    launches = len(events)
    shapes = sorted({k for _, k in events})
    steps_per_launch = shapes[-1]  # = min(chunk, steps); a shorter tail launch exists when chunk does not divide steps
    avg_launch_s = kernel_s / launches
    achieved = algorithmic_bytes_per_env_step(H) * B * args.steps / kernel_s / 1e9
    prof = pmc_profile(B, H, steps_per_launch, args.circle_radius) if len(shapes) == 1 else None
    s = m['summary']
    src = pmc_provenance() if prof is not None else None
    fresh = src is not None and not src['stale']  # the PMC record describes the kernels of this tree
    fills = m['fills_in_timed_region']
    # a call tops the scenario ring up only when the steps since the last fill exceed its depth (cn_rollout: the ring budget
    # rule), so a short timed region can contain no fill at all: value_amortised_fill charges it the steady-state share —
    # one fill (fill_ms: a 1-step call that carries one minus a 1-step call that does not, measured after the timed region on
    # the same engine) per ring_depth steps.  A region that contains its fills (fills_in_timed_region > 0) needs no correction.
    fill_s = m['fill_s']
    if fills > 0 or args.async_fill:
        amortised = total / elapsed
    elif fill_s is not None:
        amortised = total / (elapsed + fill_s * args.steps / m['ring_depth'])
    else:
        amortised = None
    out = {
        'metric': 'env-steps/sec (whole node), %d envs x %d humans, ORCA step' % (B, H),
        'value': total / elapsed, 'unit': 'env-steps/s', 'n_gpus': world, 'steps': args.steps,
        'warmup': args.warmup, 'ms_per_step': elapsed * 1e3 / args.steps, 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32 ORCA solve + f64 env step', 'data': 'synthetic',
        'value_definition': 'all ranks\' transitions / the slowest rank\'s wall time of the K batched steps (transitions, in-kernel '
                            'auto-resets, per-episode records, per-env transition counters), barrier + synchronize on both sides.  '
                            'Since round 4 the job-wide statistics of explorer.py:74-90 are computed ONCE, at the shard boundary, '
                            'outside this region (boundary_ms; value_incl_boundary charges them to the K steps).  '
                            'value_r3_definition: the same K steps with every launch leaving the job-wide statistics itself — '
                            'the definition of rounds 1-3, for round-over-round comparison.  value_amortised_fill: value with '
                            'the steady-state share of the scenario-ring fill charged when the timed region contained none.'
                            if not inkernel else 'round 3 arrangement (CROWDNAV_AMD_BENCH_INKERNEL_STATS=1): every launch leaves '
                                                 'the job-wide statistics itself',
        'config': {'workload': '%s%d batched envs x %d humans per GPU, ORCA humans + holonomic ORCA robot (visible), '
                               'circle_crossing radius %g, in-kernel auto-reset'
                               % ('BASELINE configs[1]: ' if (B, H) == (4096, 5) else "BASELINE configs[3]'s shard: " if
                                  (B, H) == (4096, 20) else '', B, H, args.circle_radius),
                   'envs_per_gpu': B, 'humans': H, 'steps_per_launch': steps_per_launch, 'launches': launches,
                   'episode_seeds': '%d + c %% %d' % (args.seed_base, args.seed_mod),
                   'records_per_env': args.records,
                   'scenario_fill': 'asynchronous (side streams, per-slot ready flags): one fill launch beside every call'
                                    if args.async_fill else
                                    'synchronous, in front of a call only when the steps since the last fill exceed the %d-deep '
                                    'ring (ring budget rule); calls of the timed region that carried one: %d of %d'
                                    % (m['ring_depth'], fills, launches),
                   'fills_in_timed_region': fills,
                   'scenario_cache': (H > 8 and args.seed_mod <= 4096 and os.environ.get('CROWDNAV_AMD_SCENARIO_CACHE', '1') != '0'),
                   'preroll_steps': args.preroll, 'full': args.full,
                   'parallelism': 'env-axis shards x%d, no collective on the step path; the job-wide statistics (record blocks, '
                                  'their all-gather on several GPUs, summary kernel) once when a run ends (boundary_ms)' % world,
                   'backend': backend if world > 1 else None, 'shared_gpu': share_gpu},
        'ranks': m['per_rank'],
        'rccl': m['rccl'],
        'summary': s,
        'roofline': {'bound': 'hbm', 'achieved': achieved, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                     'frac': achieved / HBM_PEAK_GBS, 'traffic': pmc_traffic_bytes(prof) if fresh else None,
                     'traffic_from': src if fresh else None,
                     'kernel': 'cn::rollout_fused_kernel (one cn_rollout call; + cn::ring_fill_kernel when the scenario ring needs '
                               'topping up)' if H <= 5 else
                               'cn::rollout_kernel<10> (+ cn::ring_fill_wave_kernel)',
                     'avg_launch_ms': avg_launch_s * 1e3,
                     'avg_launch_ms_note': 'HIP-event span per cn_rollout call; the opening event is recorded on the idle stream '
                                           'just before the host clock starts, so the span of the first launch includes the '
                                           'host\'s enqueue latency and can exceed ms_per_step x steps by a few us',
                     'algorithmic_bytes_per_env_step': algorithmic_bytes_per_env_step(H)},
        'issue_roofline': pmc_issue(prof, B, steps_per_launch, avg_launch_s),
        'boundary_ms': boundary * 1e3,
        'value_incl_boundary': total / (elapsed + boundary),
        'value_samples': None if not m['samples'] else {
            'n': len(m['samples']), 'min': min(v for v, _ in m['samples']),
            'median': sorted(v for v, _ in m['samples'])[len(m['samples']) // 2], 'max': max(v for v, _ in m['samples']),
            'all': [v for v, _ in m['samples']], 'ring_fills': [f for _, f in m['samples']],
            'median_without_fill': (lambda w: sorted(w)[len(w) // 2] if w else None)([v for v, f in m['samples'] if f == 0]),
            'median_with_fill': (lambda w: sorted(w)[len(w) // 2] if w else None)([v for v, f in m['samples'] if f > 0]),
            'note': 'further repetitions of the same %d warm-up + %d timed steps on the same engine, fenced like the first; '
                    '`value` is the first sample.  ring_fills: scenario-ring fills inside each repetition\'s timed region (rank 0) — a '
                    'repetition that carries one (every %d steps) is the slow mode of the spread; value_amortised_fill charges '
                    'the steady-state share' % (args.warmup, args.steps, m['ring_depth'])},
        'value_r3_definition': None if m3 is None else m3['total'] / m3['elapsed'],
        'fill_ms': None if fill_s is None else fill_s * 1e3,
        'value_amortised_fill': amortised,
        'paused_env_steps': B * args.steps * world - total,
        'episodes_finished': episodes,
        'mean_recorded_return': s[6] / max(s[1], 1.0),
        'recorded_success_rate': s[2] / max(s[1], 1.0),
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out['cpu_baseline'] = cpu_baseline(B, H)
    if args.full and rank == 0 and world == 1 and not args.no_secondary and (B, H) == (4096, 5):
        out['secondary'] = secondary(B, local_rank)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
