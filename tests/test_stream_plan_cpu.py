"""The decision of a streamed coordinate-descent run (qcqp_amd/csrc/cd_life_plan.h: stream_plan, what qcqpmi_cd_stream_reserve and
qcqpmi_cd_stream_run both consume) on the host: the named shapes of DESIGN.md section 4.1 -- the headline's factored instantiation
with every restart preloaded, the same shape without the factor and through the round-4 kernel, MAXCUT n = 2000 on seven multiplying
waves, the limits n = 32 / 2304 / 2320 / 4096, three-block problems, several classes, a diagonal of mixed sign, the factor's rank, the
preloaded restarts against their budget -- and the invariants of a plan over 1 <= NB <= 260 and the switches (an unsupported plan
reserves nothing, the factored instantiation is <3, cs 0>, the workgroups and the preloaded restarts stay inside their limits).
tests/host/stream_plan_selftest.cpp, built with the host compiler: no HIP, and the switches are passed in, never read from the
environment.  tests/stream_plan_cases.py is the table's share that tests/test_gpu_stream_plan.py holds the GPU to."""
import os
import shutil
import subprocess

import pytest

from stream_plan_cases import KERNEL_NAMES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cxx():
    c = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++')
    if not c:
        pytest.skip('no host compiler')
    return c


def test_named_shapes_and_invariants_of_the_plan(cxx, tmp_path):
    exe = str(tmp_path / 'stream_plan_selftest')
    p = subprocess.run([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-I' + os.path.join(REPO, 'qcqp_amd', 'csrc'), '-o', exe,
                        os.path.join(REPO, 'tests', 'host', 'stream_plan_selftest.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    env = {k: v for k, v in os.environ.items() if not k.startswith('QCQPMI_')}
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode().strip()
    assert r.returncode == 0 and out.startswith('ok '), out
    assert int(out.split()[1]) >= 10000000, out


def test_gpu_table_is_the_selftests():
    """Every kernel name the GPU test expects stands in the selftest's table."""
    src = open(os.path.join(REPO, 'tests', 'host', 'stream_plan_selftest.cpp')).read()
    for name in set(KERNEL_NAMES.values()):
        assert '"%s"' % name in src, name
