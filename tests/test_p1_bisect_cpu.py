"""The fused bisection of the band class's phase-1 visit (qcqp_amd/csrc/p1_bisect.h) on the host: its fast first phase followed by
the general loop must leave every element in the state the general loop alone leaves it in -- ss, es, sp, it, itp, pending, bit for
bit -- on 1e7 random violations in [0, 1e9] (log-uniform and uniform, fused in random pairs), on the edge values of
viol - viol_tol (<= 0, denormal, 1e-300, tol and its neighbours, huge, NaN), and wherever a midpoint of the bisection falls within a
few guards of 0 (at the first step and at every later one up to the 41st), for (tol, viol_tol) = (1e-4, 1e-2) and (1e-6, 1e-3) and
r = -1 and -4.  tests/host/p1_bisect_selftest.cpp, built with the host compiler and -ffp-contract=off (the device build's setting)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cxx():
    c = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++')
    if not c:
        pytest.skip('no host compiler')
    return c


def build(cxx, tmp_path, extra=()):
    exe = str(tmp_path / 'p1_bisect_selftest')
    p = subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I' + os.path.join(REPO, 'qcqp_amd', 'csrc'), '-o', exe,
                        os.path.join(REPO, 'tests', 'host', 'p1_bisect_selftest.cpp')] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    return exe


def test_fast_phase_then_general_loop_equals_general_loop(cxx, tmp_path):
    r = subprocess.run([build(cxx, tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode().strip()
    assert r.returncode == 0 and out.startswith('ok '), out
    assert int(out.split()[1]) >= 10000000, out


def test_switch_builds_the_general_loop_alone(cxx, tmp_path):
    """-DQCQPMI_P1_FASTBISECT=0 (the A/B build) compiles, and the program says that it has nothing to compare."""
    r = subprocess.run([build(cxx, tmp_path, ['-DQCQPMI_P1_FASTBISECT=0'])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 2, r.stdout.decode()
