"""Per-function comparison of the device assembly of two revisions: which kernels a source change really touched.

    python scripts/kernel_asm_diff.py [--base REV] [--tu UNIT|env|sarl|train|plan|all] [-v]

Compiles the translation units of REV (default HEAD; taken from git into a temporary directory) and of the working tree — every
*.hip file of a tree's crowdnav_amd/csrc is one — with the Makefile's flags plus --cuda-device-only -S (cross-compiles without a
GPU), up to 8 at a time, splits the assembly into functions and POOLS the functions of all units of a revision by mangled name:
a kernel that moved from one unit to another is compared with itself, not reported as gone plus new.  A name that two units of one
revision define is an error (a non-template kernel in a header that two units include would not link either).  Compares the
instruction streams with comments, directives and the function index of local labels stripped.  Prints one line per function
that differs (instruction count before -> after), a summary, and exits 1 if any differ.  -v lists the identical ones as well.
--tu narrows both sides to one unit by its file's basename, or to env (crowdnav_amd), sarl (every sarl_* unit but sarl_train),
train (sarl_train), plan; default sarl.  The assembly files stay under build/asm/ (the base revision's are reused by commit hash).
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-fno-slp-vectorize',
         '--cuda-device-only', '-S']
ASM = os.path.join(ROOT, 'build', 'asm')
ALIASES = {'env': lambda u: u == 'crowdnav_amd', 'sarl': lambda u: u.startswith('sarl_') and u != 'sarl_train',
           'train': lambda u: u == 'sarl_train', 'all': lambda u: True}


def units_of(tree, tu='all'):
    """Basenames of the tree's translation units (its own *.hip files) that --tu selects."""
    csrc = os.path.join(tree, 'crowdnav_amd', 'csrc')
    want = ALIASES.get(tu, lambda u: u == tu)
    return sorted(f[:-4] for f in os.listdir(csrc) if f.endswith('.hip') and want(f[:-4]))


def compile_units(tree, units, out_of):
    """unit -> out_of(unit), the missing ones compiled up to 8 at a time."""
    csrc = os.path.join(tree, 'crowdnav_amd', 'csrc')

    def one(u):
        return u, subprocess.run(['/opt/rocm/bin/hipcc'] + FLAGS + [u + '.hip', '-o', out_of(u)], cwd=csrc, stderr=subprocess.PIPE, text=True)
    with ThreadPoolExecutor(max_workers=8) as pool:
        for u, r in pool.map(one, units):
            if r.returncode:  # (warnings of a compile that succeeds are the build's business)
                sys.exit('hipcc failed on %s.hip of %s:\n%s' % (u, tree, r.stderr))


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


def pool_functions(paths):
    """The functions of all assembly files of ONE revision by mangled name; ValueError if two files define the same name."""
    pooled, where = {}, {}
    for path in paths:
        for name, body in functions(path).items():
            if name in pooled:
                raise ValueError('%s is defined in two units of one revision: %s and %s' % (name, where[name], path))
            pooled[name], where[name] = body, path
    return pooled


def compare(old, new):
    """(names whose streams are identical, names that differ — changed, gone or new), each sorted."""
    same = sorted(k for k in old if k in new and old[k] == new[k])
    return same, sorted((set(old) | set(new)) - set(same))


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
    sha = subprocess.check_output(['git', 'rev-parse', '--short=12', base], cwd=ROOT, text=True).strip()
    os.makedirs(ASM, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:  # the base revision's own files say what its units are
        tar = subprocess.Popen(['git', 'archive', sha, 'crowdnav_amd/csrc', 'include'], cwd=ROOT, stdout=subprocess.PIPE)
        subprocess.check_call(['tar', '-x', '-C', tmp], stdin=tar.stdout)
        tar.wait()
        old_units = units_of(tmp, tu)
        old_s = lambda u: os.path.join(ASM, '%s_%s.s' % (sha, u))  # noqa: E731
        compile_units(tmp, [u for u in old_units if not os.path.exists(old_s(u))], old_s)
    new_units = units_of(ROOT, tu)
    new_s = lambda u: os.path.join(ASM, 'worktree_%s.s' % u)  # noqa: E731
    compile_units(ROOT, new_units, new_s)
    if not old_units and not new_units:
        sys.exit('--tu %s names no unit of either revision' % tu)
    try:
        old, new = pool_functions(map(old_s, old_units)), pool_functions(map(new_s, new_units))
    except ValueError as err:
        sys.exit(str(err))
    same, differ = compare(old, new)
    names = demangle(sorted(set(old) | set(new)))
    for k in sorted(names, key=names.get):
        if k in differ:
            a = '%6d' % count(old[k]) if k in old else '     -'
            b = '%-6d' % count(new[k]) if k in new else '-     '
            print('  DIFFERS  %s -> %s %s' % (a, b, names[k]))
        elif verbose:
            print('  same     %6d          %s' % (count(old[k]), names[k]))
    print('%s: %d functions of %s (%s) identical in the working tree (%s), %d differ' % (
        tu, len(same), sha, ' '.join(old_units) or '-', ' '.join(new_units) or '-', len(differ)))
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
