"""Per-kernel register / spill / LDS table of libcrowdnav_amd.so's code object, from hipcc's own resource report
(-Rpass-analysis=kernel-resource-usage; cross-compiles without a GPU).

    python scripts/kernel_resources.py [--tu UNIT|env|sarl|train|plan|all] [filter-regex] [-D...]      # extra -D flags go to hipcc

--tu names the translation units — the *.hip files of crowdnav_amd/csrc — by a file's basename or as kernel_asm_diff.py does:
env (default) = crowdnav_amd.hip, sarl = every sarl_* unit but sarl_train (the value-network kernels), train = sarl_train.hip
(the device SGD step), plan = plan.hip (the CEM / MPPI planners' kernels), all.  The rows of several units follow each other.
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_asm_diff import ROOT, units_of  # noqa: E402


def report(extra=(), unit='crowdnav_amd'):
    src = os.path.join(ROOT, 'crowdnav_amd', 'csrc', unit + '.hip')
    cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-slp-vectorize',
           '-fno-fast-math', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', '/dev/null'] + list(extra)
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, cwd=os.path.dirname(src)).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r'remark: +(.*?): (.*?) \[-Rpass', line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k in ('Function Name', 'Name'):
            cur = {'name': v}
            rows.append(cur)
        elif cur is not None:
            cur[k] = v
    return rows


def demangle(names):
    out = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE, text=True).stdout
    return [re.sub(r'\(.*', '', n).replace('void ', '') for n in out.splitlines()]


def main():
    argv, tu = sys.argv[1:], 'env'
    if '--tu' in argv:
        i = argv.index('--tu')
        tu = argv[i + 1]
        del argv[i:i + 2]
    units = units_of(ROOT, tu)
    if not units:
        sys.exit('--tu takes env, sarl, train, plan, all or one of: ' + ', '.join(units_of(ROOT)))
    args = [a for a in argv if not a.startswith('-D')]
    extra = [a for a in argv if a.startswith('-D')]
    pat = re.compile(args[0]) if args else None
    rows = [r for u in units for r in report(extra, u)]
    if not rows:
        sys.exit('no kernel resource remarks: the compile failed (run the hipcc command by hand to see why)')
    names = demangle([r['name'] for r in rows])
    print('%-52s %5s %5s %5s %7s %7s %8s %4s %7s' % ('kernel', 'SGPR', 'VGPR', 'AGPR', 'sp.SGPR', 'sp.VGPR', 'scratch', 'occ', 'LDS'))
    for r, n in zip(rows, names):
        if pat and not pat.search(n):
            continue
        g = lambda *ks: next((r[k] for k in ks if k in r), '-')  # noqa: E731
        print('%-52s %5s %5s %5s %7s %7s %8s %4s %7s' % (
            n[-52:], g('TotalSGPRs', 'SGPRs'), g('VGPRs'), g('AGPRs'), g('SGPRs Spill'), g('VGPRs Spill'),
            g('ScratchSize [bytes/lane]'), g('Occupancy [waves/SIMD]'), g('LDS Size [bytes/block]')))


if __name__ == '__main__':
    main()
