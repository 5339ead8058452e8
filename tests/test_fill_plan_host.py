"""The host's rule for filling the scenario ring (crowdnav_amd/csrc/fill_plan.h) without a GPU: the header includes nothing of
HIP, so tests/fill_plan_check.cpp — a stand-alone program — is compiled with the host compiler and run.  It checks the rule's
decisions on hand-written call sequences (bench.py's two shapes among them) and brute-forces, for ring depths 1, 2, 3 and 48 and
random call lengths of 1..200, that a launch sees the synchronous rule's fill level wherever that rule fills and at least its
own length elsewhere, that every ordinal below the level is resident, and that a fill running beside a launch never writes a
slot the launch may still read — whichever side of the launch's end it reads the env's episode word on.  The model executes
the hand-over of the two level buffers from the plan's own decisions (a fill beside a launch writes the buffer the launch does
not read; the next launch reads the one it wrote; once per fill), and every sequence runs twice from one seed, with and without
settles between the calls: the same decisions and the same levels."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_fill_plan_decisions_and_ring_invariants(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler found (g++, c++, clang++)')
    exe = str(tmp_path / 'fill_plan_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'crowdnav_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'fill_plan_check.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith('ok '), r.stdout
    assert int(r.stdout.split()[1]) > 100000  # the brute force ran
