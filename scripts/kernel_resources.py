"""Per-kernel register / spill / LDS table of libcrowdnav_amd.so's code object, from hipcc's own resource report
(-Rpass-analysis=kernel-resource-usage; cross-compiles without a GPU).

    python scripts/kernel_resources.py [--tu env|sarl|train|plan] [filter-regex] [-D...]      # extra -D flags go to hipcc

--tu names the translation unit: env (default) = crowdnav_amd.hip, sarl = sarl_abi.hip (the value-network kernels),
train = sarl_train.hip (the device SGD step), plan = plan.hip (the CEM / MPPI planners' kernels).
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUS = {'env': 'crowdnav_amd.hip', 'sarl': 'sarl_abi.hip', 'train': 'sarl_train.hip', 'plan': 'plan.hip'}


def report(extra=(), tu='env'):
    src = os.path.join(ROOT, 'crowdnav_amd', 'csrc', TUS[tu])
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
        if tu not in TUS:
            sys.exit('--tu takes one of: ' + ', '.join(TUS))
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith('-D')]
    extra = [a for a in argv if a.startswith('-D')]
    pat = re.compile(args[0]) if args else None
    rows = report(extra, tu)
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
