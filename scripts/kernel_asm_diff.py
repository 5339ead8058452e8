"""Per-function comparison of the device assembly of two revisions: which kernels a source change really touched.

    python scripts/kernel_asm_diff.py [--base REV] [--tu env|sarl|train|plan|all] [-v]

Compiles the translation unit(s) of REV (default HEAD; taken from git into a temporary directory) and of the working tree with the
Makefile's flags plus --cuda-device-only -S (cross-compiles without a GPU; sarl_abi.hip takes ~1.5 minutes), splits the
assembly into functions and compares their instruction streams with comments, directives and the function index of local labels
stripped.  Prints one line per function that differs (instruction count before -> after), a summary, and exits 1 if any differ.
A translation unit REV does not have yet counts as empty there: all its functions are listed as new.
-v lists the identical ones as well.  The assembly files stay under build/asm/ (the base revision's are reused by commit hash).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUS = {'env': 'crowdnav_amd.hip', 'sarl': 'sarl_abi.hip', 'train': 'sarl_train.hip', 'plan': 'plan.hip'}
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-fno-slp-vectorize',
         '--cuda-device-only', '-S']
ASM = os.path.join(ROOT, 'build', 'asm')


def compile_tu(tree, tu, out):
    csrc = os.path.join(tree, 'crowdnav_amd', 'csrc')
    if not os.path.exists(os.path.join(csrc, TUS[tu])):  # a translation unit added since: no functions
        open(out, 'w').close()
        return
    r = subprocess.run(['/opt/rocm/bin/hipcc'] + FLAGS + [TUS[tu], '-o', out], cwd=csrc, stderr=subprocess.PIPE, text=True)
    if r.returncode:  # (warnings of a compile that succeeds are the build's business)
        sys.exit('hipcc failed on %s of %s:\n%s' % (TUS[tu], tree, r.stderr))


def functions(path):
    """{name: [instruction lines]} of every function (kernels and called device functions) of an assembly file."""
    funcs, cur = {}, None
    types = set()
    lines = open(path).read().splitlines()
    for line in lines:
        m = re.match(r'\s*\.type\s+(\S+),@function', line)
        if m:
            types.add(m.group(1))
    for line in lines:
        m = re.match(r'(\S+):', line)
        if m and m.group(1) in types:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if re.match(r'\.Lfunc_end\d+:', line):
            cur = None
            continue
        text = line.split(';')[0].strip()
        if not text or (text.startswith('.') and not text.endswith(':')):
            continue  # comment or directive
        cur.append(re.sub(r'\.L(BB|tmp|JTI)\d+_', r'.L\1_', text))
    return funcs


def demangle(names):
    out = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return dict(zip(names, (re.sub(r'\(.*', '', n).replace('void ', '') for n in out)))


def count(body):
    return sum(1 for l in body if not l.endswith(':'))


def main():
    argv = sys.argv[1:]
    verbose = '-v' in argv
    base = argv[argv.index('--base') + 1] if '--base' in argv else 'HEAD'
    tu = argv[argv.index('--tu') + 1] if '--tu' in argv else 'sarl'
    tus = list(TUS) if tu == 'all' else [tu]
    sha = subprocess.check_output(['git', 'rev-parse', '--short=12', base], cwd=ROOT, text=True).strip()
    os.makedirs(ASM, exist_ok=True)
    differ = 0
    for t in tus:
        old_s, new_s = os.path.join(ASM, '%s_%s.s' % (sha, t)), os.path.join(ASM, 'worktree_%s.s' % t)
        if not os.path.exists(old_s):
            with tempfile.TemporaryDirectory() as tmp:
                tar = subprocess.Popen(['git', 'archive', sha, 'crowdnav_amd/csrc', 'include'], cwd=ROOT, stdout=subprocess.PIPE)
                subprocess.check_call(['tar', '-x', '-C', tmp], stdin=tar.stdout)
                tar.wait()
                compile_tu(tmp, t, old_s)
        compile_tu(ROOT, t, new_s)
        old, new = functions(old_s), functions(new_s)
        names = demangle(sorted(set(old) | set(new)))
        same = 0
        for k in sorted(names, key=names.get):
            if k in old and k in new and old[k] == new[k]:
                same += 1
                if verbose:
                    print('  same     %6d          %s' % (count(old[k]), names[k]))
                continue
            differ += 1
            a = '%6d' % count(old[k]) if k in old else '     -'
            b = '%-6d' % count(new[k]) if k in new else '-     '
            print('  DIFFERS  %s -> %s %s' % (a, b, names[k]))
        print('%s (%s): %d functions identical to %s, %d differ' % (t, TUS[t], same, sha, len(names) - same))
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
