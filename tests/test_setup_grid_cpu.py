"""The device-side setup of batched ADMM without a GPU, the long part (tests/test_admm_setup_cpu.py has the rest and says why this
is a file of its own): the NumPy restatement of the two setup kernels (tests/admm_setup_cases.py) satisfies, on every case of the GPU
test, what the project already asserts of the host setup (tests/test_admm_batch_cpu.py: rho to 1e-12 of the oracle's auto_rho(),
Minv_b rhs to 1e-12 of the oracle's Cholesky solve, Minv_b exactly symmetric) and stays within the recorded distance of eigvalsh; the
rule on the diagonal and the zero family bit for bit; and tests/host/admm_setup_selftest.cpp holds the scalar pieces of
csrc/admm_setup_rule.h against long-double references (host compiler, -ffp-contract=off; once more under ASan + UBSan)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import admm_setup_cases as asc
from conftest import REPO


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name,n', [(name, n) for name in asc.FAMILIES for n in asc.SIZES + asc.SIZES_WIDE],
                         ids=lambda v: str(v))
def test_restatement_against_the_oracle_and_eigvalsh(orc, name, n):
    """The three problems of B = 3 (B = 1 is the first of them): the statements of
    tests/test_admm_batch_cpu.py::test_rho_rule_and_batched_inverse_agree_with_the_oracle with its tolerances, and lambda_min within
    LMIN_MEASURED |P0|_F of eigvalsh -- the figure the GPU test's bound is ten times of."""
    from qcqp_amd import batch
    rs = np.random.RandomState(n)
    for b in range(max(asc.BS)):
        funcs, P0, m = asc.problem(name, n, b)
        r = asc.restated(name, n, b)
        fro, ref = float(np.linalg.norm(P0)), float(np.linalg.eigvalsh(P0)[0])
        assert r['status'] == 0 and r['sweeps'] <= 16, (b, r['status'], r['sweeps'])
        assert abs(r['lambda_min'] - ref) <= asc.LMIN_MEASURED * fro, (b, abs(r['lambda_min'] - ref) / fro)
        assert r['rho'] == asc.rho_rule(r['lambda_min'], m)
        auto = orc.Problem(funcs).auto_rho()
        if abs(ref) > asc.LMIN_GATE * fro:                  # clear of the rule's jump
            assert abs(r['rho'] - auto) <= asc.RHO_RTOL * auto, (b, r['rho'], auto)
        else:                                               # on this grid only P0 = 0 is not: the zero family, MAXCUT without an edge
            assert fro == 0.0 and (name == 'zero' or (name == 'cut' and n <= 2))
            assert r['lambda_min'] == 0.0 and r['sweeps'] == 0 and r['rho'] == 50.0 * (1.0 / m) == auto
            assert np.array_equal(r['Minv'], np.eye(n) * (1.0 / (2.0 * (r['rho'] * m))))
        if name == 'diag':                                  # the solvers leave a diagonal matrix alone: the host's bits
            assert r['rho'] == batch.admm_rhos(P0[None], m)[0] and r['lambda_min'] == ref
        assert np.array_equal(r['Minv'], r['Minv'].T)
        rhs = rs.randn(n)
        assert asc.ab.rel(r['Minv'].dot(rhs), asc.cholesky_solve(P0, auto, m, rhs)) <= asc.SOLVE_RTOL, b


# ------------------------------------------------------------------ the scalar pieces on the host
@pytest.fixture(scope='module')
def cxx():
    c = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++')
    if not c:
        pytest.skip('no host compiler')
    return c


def _selftest(cxx, tmp_path, extra=()):
    exe = str(tmp_path / 'admm_setup_selftest')
    p = subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I' + os.path.join(REPO, 'tests', 'host', 'hip_stub'),
                        '-I' + os.path.join(REPO, 'qcqp_amd', 'csrc'), '-o', exe, os.path.join(REPO, 'tests', 'host', 'admm_setup_selftest.cpp')]
                       + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode().strip()
    assert r.returncode == 0 and out.startswith('ok '), out
    return int(out.split()[1])


def test_rule_and_weight_against_long_double(cxx, tmp_path):
    assert _selftest(cxx, tmp_path) >= 1000000


def test_rule_and_weight_under_sanitizers(cxx, tmp_path):
    """The same stand-alone program under AddressSanitizer + UBSan (host code only; nothing is loaded into Python)."""
    assert _selftest(cxx, tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']) >= 1000000
