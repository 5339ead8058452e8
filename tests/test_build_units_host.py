"""The library's translation units are the *.hip files of crowdnav_amd/csrc, named nowhere else: the Makefile compiles each of
them, and scripts/kernel_asm_diff.py pools the device functions of a revision's units by mangled name before it compares two
revisions — a kernel that moved between units is compared with itself, and a name that two units of one revision define is an
error.  The pooling on small assembly texts written here; no compiler, no GPU."""
import importlib.util
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'crowdnav_amd', 'csrc')


def _tool():
    spec = importlib.util.spec_from_file_location('kernel_asm_diff', os.path.join(ROOT, 'scripts', 'kernel_asm_diff.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _asm(index, name, body):
    """One function as hipcc -S prints it: its .type line, the label, local labels that carry the function's index, the end label."""
    lines = ['\t.type\t%s,@function' % name, '%s:                                   ; @%s' % (name, name), '; %%bb.0:']
    lines += ['\t%s' % b for b in body[:2]] + ['.LBB%d_1:' % index] + ['\t%s' % b for b in body[2:]]
    lines += ['\ts_cbranch_scc1 .LBB%d_1                   ; a comment' % index, '\ts_endpgm', '.Lfunc_end%d:' % index, '\t.size\t%s, .Lfunc_end%d-%s' % (name, index, name)]
    return '\n'.join(lines) + '\n'


A = ['s_load_dwordx2 s[0:1], s[4:5], 0x0', 'v_mov_b32_e32 v1, 0', 'v_add_f32_e32 v1, v1, v0', 's_cmp_lg_u32 s2, 0']
B = ['s_load_dword s0, s[4:5], 0x8', 'v_lshlrev_b32_e32 v0, 2, v0', 'v_mul_f32_e32 v1, v0, v0', 's_cmp_eq_u32 s0, 1']
B_CHANGED = B[:2] + ['v_fma_f32 v1, v0, v0, v0'] + B[3:]


def _write(tmp_path, name, *functions):
    path = tmp_path / name
    path.write_text('\t.text\n' + ''.join(_asm(i, n, body) for i, (n, body) in enumerate(functions)))
    return str(path)


def test_a_function_that_moved_between_units_is_identical_and_a_changed_one_differs(tmp_path):
    tool = _tool()
    # before: one unit holds both kernels.  after: _Z1bv moved to a unit of its own (so its local labels carry another index)
    old = tool.pool_functions([_write(tmp_path, 'old_abi.s', ('_Z1av', A), ('_Z1bv', B))])
    moved = tool.pool_functions([_write(tmp_path, 'new_abi.s', ('_Z1av', A)), _write(tmp_path, 'new_reg.s', ('_Z1bv', B))])
    assert set(old) == set(moved) == {'_Z1av', '_Z1bv'} and tool.count(old['_Z1bv']) == len(B) + 2
    assert tool.compare(old, moved) == (['_Z1av', '_Z1bv'], [])
    changed = tool.pool_functions([_write(tmp_path, 'chg_abi.s', ('_Z1av', A)), _write(tmp_path, 'chg_reg.s', ('_Z1bv', B_CHANGED))])
    assert tool.compare(old, changed) == (['_Z1av'], ['_Z1bv'])
    # gone or new is a difference too, never silence
    only_a = tool.pool_functions([_write(tmp_path, 'only_a.s', ('_Z1av', A))])
    assert tool.compare(old, only_a) == (['_Z1av'], ['_Z1bv']) and tool.compare(only_a, old) == (['_Z1av'], ['_Z1bv'])


def test_a_name_defined_in_two_units_of_one_revision_is_an_error(tmp_path):
    tool = _tool()
    first, second = _write(tmp_path, 'abi.s', ('_Z1av', A), ('_Z1bv', B)), _write(tmp_path, 'reg.s', ('_Z1bv', B))
    with pytest.raises(ValueError) as err:
        tool.pool_functions([first, second])
    assert '_Z1bv' in str(err.value) and first in str(err.value) and second in str(err.value)


def test_the_tools_take_a_trees_units_from_its_hip_files(tmp_path):
    tool = _tool()
    csrc = tmp_path / 'crowdnav_amd' / 'csrc'
    csrc.mkdir(parents=True)
    for name in ('crowdnav_amd.hip', 'sarl_abi.hip', 'sarl_new.hip', 'sarl_train.hip', 'plan.hip', 'sarl_kernels.h'):
        (csrc / name).write_text('')
    assert tool.units_of(str(tmp_path)) == ['crowdnav_amd', 'plan', 'sarl_abi', 'sarl_new', 'sarl_train']
    assert tool.units_of(str(tmp_path), 'sarl') == ['sarl_abi', 'sarl_new'] and tool.units_of(str(tmp_path), 'env') == ['crowdnav_amd']
    assert tool.units_of(str(tmp_path), 'train') == ['sarl_train'] and tool.units_of(str(tmp_path), 'sarl_new') == ['sarl_new']
    assert tool.units_of(str(tmp_path), 'nothing') == []


def test_make_names_a_compile_line_for_every_hip_file():
    units = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith('.hip'))
    assert 4 <= len(units) <= 16  # (all of them compile side by side)
    # -B: whatever is built already; the lines of the product objects, then of an experiment build
    for goal, obj in ((['all'], '%s.o'), (['exp', 'NAME=unitcheck'], 'obj_unitcheck_%s.o')):
        out = subprocess.run(['make', '-n', '-B', '-C', CSRC] + goal, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode == 0, out.stdout
        compiles = [l for l in out.stdout.splitlines() if 'hipcc' in l and ' -c ' in l]
        for u in units:
            assert sum(1 for l in compiles if ' -c %s.hip ' % u in l and l.endswith(obj % u)) == 1, (u, out.stdout)
        assert len(compiles) == len(units)
