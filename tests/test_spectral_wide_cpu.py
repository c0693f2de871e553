"""The wide spectral suggest (qcqpmi_spectral_batch, QCQPBatch.suggest(SPECTRAL, wide=True)) without a GPU: the symbol is declared,
bound and exported within ABI 6 and the new headers reach the units that build them; the NumPy restatement of the wide kernel
(tests/spectral_wide_cases.py) agrees with eigvalsh and with the independent solver of tests/spectral_batch_cases.py on every case of
the GPU test; the one-sided Jacobi of the restatement on its own (orthogonality, the padding coordinate, A = 0, a fully degenerate
spectrum, exact ties); the facade's choice of entry point on a recording stand-in; and tests/host/spectral_wide_selftest.cpp holds
hestenes_rotation of csrc/spectral_solve.h against long-double references (host compiler, -ffp-contract=off; once more under ASan +
UBSan).  On the commit before the feature the symbol, the keyword's effect and the rotation are missing."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import spectral_batch_cases as sc
import spectral_wide_cases as wc
from conftest import REPO

SYMBOL = 'qcqpmi_spectral_batch'


def test_symbol_in_header_binding_library_and_build_units():
    with open(os.path.join(REPO, 'include', 'qcqp_mi.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+%s\s*\(' % SYMBOL, header)
    assert re.search(r'#define\s+QCQPMI_ABI_VERSION\s+6\b', header)
    from qcqp_amd import _build, _ffi
    proto = {p[0]: p for p in _ffi.PROTOTYPES}
    assert proto[SYMBOL][1:] == proto['qcqpmi_spectral_small_batch'][1:] and len(proto[SYMBOL][2]) == 17
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL) and lib.qcqpmi_abi_version() == 6
    # the wide kernel is built in the unit of the narrow one; the driver sees the launcher's declarations only
    reach = {h: sorted(u for u in _build.TRANSLATION_UNITS if os.path.join(_build.SRC, h) in _build.unit_sources(u))
             for h in ('spectral_wide.h', 'spectral_wide_kernel.h', 'jacobi_wide.h')}
    assert reach['spectral_wide.h'] == ['capi_small.hip', 'spectral_small.hip']
    assert reach['spectral_wide_kernel.h'] == ['spectral_small.hip'] and reach['jacobi_wide.h'] == ['spectral_small.hip']
    # the eigen-solver's header stands on its own: the shared device helpers and the scalar pieces, nothing of the spectral kernels
    with open(os.path.join(_build.SRC, 'jacobi_wide.h')) as f:
        assert sorted(re.findall(r'#include "([^"]+)"', f.read())) == ['dev_util.h', 'spectral_solve.h']
    assert lib.qcqpmi_spectral_batch(None, 1, None, None, None, None, 0, 1, 30, 1e-15, None, None, None, None, None, None, None) == -1


def test_lds_of_the_wide_kernel_fits_a_compute_unit():
    """(n2 (n2 + 1) + 5 * 128) doubles: 137 216 bytes at n = 128, below the 160 KiB of a compute unit; four images at n = 65.  The
    narrow solver's two arrays (jacobi_small.h: 2 * 65 n2 doubles at a stride that only reaches 64 columns) would need 2 n2^2."""
    lds = lambda n: (((n + 1) & ~1) * (((n + 1) & ~1) + 1) + 5 * 128) * 8
    assert lds(128) == 137216 and lds(128) <= 160 * 1024 < 2 * 128 * 128 * 8
    assert lds(65) == 40496 and 160 * 1024 // lds(65) == 4
    with open(os.path.join(REPO, 'qcqp_amd', 'csrc', 'spectral_wide.h')) as f:
        text = f.read()
    assert '137 216' in text and '40 496' in text


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', sc.FAMILIES)
def test_restatement_agrees_with_eigvalsh_and_the_independent_solver(name):
    """Every case of the GPU test, B = 2: the bound to 1e-9 (1 + |f|) -- the project's parity tolerance -- and the eigenvalues (Rayleigh
    quotients) to 1e-12 |A|_F of eigvalsh, the GPU test's bound: their error is O(n eps |A|_F), 3e-14 |A|_F at n = 128.  The
    restatement's status is 0 within 16 sweeps; the families take the branch they were built for; U'U = I to 1e-14."""
    want = {'maxcut': {2}, 'ident': {2}, 'nearhard': {1}, 'bls': {1}, 'eqpp': {1}, 'box11_in': {0}, 'box01_in': {0}, 'box11_out': {1},
            'box01_out': {1}}
    for n in wc.SIZES_WIDE:
        fl, P0s, q0s, r0s, aggs, relop, _ = sc.case(name, n, 2)
        for b, r in enumerate(wc.restated(name, n, 2)):
            ind = sc.independent(P0s[b], q0s[b], r0s[b], aggs[b], relop)
            lam = np.linalg.eigvalsh(0.5 * (r['A'] + r['A'].T))
            assert r['status'] == 0 and r['sweeps'] <= 16, (name, n, b, r['sweeps'])
            assert np.max(np.abs(r['U'].T.dot(r['U']) - np.eye(r['U'].shape[0]))) <= 1e-14, (name, n, b)
            assert abs(r['bound'] - ind['bound']) <= 1e-9 * (1.0 + abs(ind['bound'])), (name, n, b, r['bound'], ind['bound'])
            assert np.max(np.abs(r['lam'] - lam)) <= 1e-12 * np.linalg.norm(r['A']), (name, n, b)
            assert r['branch'] == ind['branch'], (name, n, b)
            if name in want:
                assert r['branch'] in want[name], (name, n, b, r['branch'])
            if name in sc.REGULAR:
                assert np.max(np.abs(r['x'] - ind['x'])) <= 1e-9 * (1.0 + np.max(np.abs(ind['x']))), (name, n, b)


def test_rayleigh_quotients_beat_the_shifted_norms():
    """Why the kernel re-reads A for the eigenvalues: |g_k| - c carries the rounding of c = 2 |A|_F against the eigenvalue.  On a
    random symmetric matrix at n = 128 the Rayleigh quotients are within 2^-46 max |lam| of eigvalsh -- the gap at which the
    hard-case rule puts eigenvalues into the lowest eigenspace -- and closer than the shifted norms."""
    rs = np.random.RandomState(2)
    M = rs.randn(128, 128)
    A = 0.5 * (M + M.T)
    ref = np.linalg.eigvalsh(A)
    n2 = 128
    G = A.copy()
    fro2 = wc.wave_sum2(np.sum(G * G, axis=0))
    c = 2.0 * np.sqrt(fro2)
    U, sweeps, conv, c2 = wc.jacobi_wide(A)
    assert conv and c2 == c and sweeps <= 16
    rayleigh = np.sort(np.einsum('ik,ik->k', U, A.dot(U)))
    norms = np.sort(np.linalg.norm((A + c * np.eye(n2)).dot(U), axis=0) - c)
    top = np.max(np.abs(ref))
    e_r, e_n = np.max(np.abs(rayleigh - ref)) / top, np.max(np.abs(norms - ref)) / top
    print('Rayleigh %.2e, shifted norms %.2e of max |lam|' % (e_r, e_n))
    assert e_r <= sc.HARD_THR and e_r < e_n


@pytest.mark.parametrize('n', [1, 2, 5, 65, 127])
def test_padding_coordinate_stays_put(n):
    rs = np.random.RandomState(n)
    M = rs.randn(n, n)
    U, sweeps, conv, _ = wc.jacobi_wide(0.5 * (M + M.T))
    n2 = (n + 1) & ~1
    assert conv and U.shape == (n2, n2)
    if n2 != n:
        e = np.zeros(n2)
        e[n] = 1.0
        assert np.array_equal(U[:, n], e) and np.array_equal(U[n, :], e)
    assert np.max(np.abs(U.T.dot(U) - np.eye(n2))) <= 1e-14


def test_zero_matrix_is_a_case_of_its_own():
    for n in (1, 65, 128):
        U, sweeps, conv, c = wc.jacobi_wide(np.zeros((n, n)))
        assert conv and sweeps == 0 and c == 0.0 and np.array_equal(U, np.eye((n + 1) & ~1))
    # P0 = 0 with q0 != 0 on the sphere |x|^2 = n: x = -sqrt(n) q0 / |q0|
    n = 65
    q0 = np.random.RandomState(1).randn(n)
    r = wc.restate(np.zeros((n, n)), q0, 0.25, np.concatenate([np.ones(n), np.zeros(n), [-float(n)]]), '==')
    assert r['status'] == 0 and r['sweeps'] == 0 and r['branch'] == 1 and np.all(r['lam'] == 0.0)
    assert np.max(np.abs(r['x'] + np.sqrt(n) * q0 / np.linalg.norm(q0))) <= 1e-12 * np.sqrt(n)
    assert abs(r['bound'] - (0.25 - np.sqrt(n) * np.linalg.norm(q0))) <= 1e-12 * (1 + np.sqrt(n) * np.linalg.norm(q0))


@pytest.mark.parametrize('n', [65, 128])
def test_fully_degenerate_spectrum_and_exact_ties(n):
    """A = I: the columns of G = (1 + c) I are orthogonal from the start: one sweep, nothing rotates, U = I, every eigenvalue exactly 1
    and rank = index.  A = diag with exact ties: the same, and lam ascending through the rank with ties in index order.  A tie that
    is not diagonal (two copies of one 2 x 2 block): equal eigenvalues to rounding, orthogonal vectors."""
    U, sweeps, conv, _ = wc.jacobi_wide(np.eye(n))
    assert conv and sweeps == 1 and np.array_equal(U, np.eye((n + 1) & ~1))
    r = wc.restate(np.eye(n), np.zeros(n), 0.0, np.concatenate([np.ones(n), np.zeros(n), [-float(n)]]), '==')
    assert r['branch'] == 2 and np.array_equal(r['lam'], np.ones(n)) and abs(r['bound'] - n) <= 1e-12 * n
    dvals = np.array([3.0, -1.0, 3.0, -1.0, 0.5] * 26)[:n]
    U, sweeps, conv, _ = wc.jacobi_wide(np.diag(dvals))
    assert conv and sweeps == 1 and np.array_equal(U[:n, :n], np.eye(n))
    r = wc.restate(np.diag(dvals), np.ones(n), 0.0, np.concatenate([np.ones(n), np.zeros(n), [-float(n)]]), '==')
    assert np.array_equal(r['lam'], np.sort(dvals)) and r['status'] == 0
    blk = np.array([[2.0, 1.0], [1.0, -1.0]])
    m = n // 2
    A = np.kron(np.eye(m), blk)
    U, sweeps, conv, _ = wc.jacobi_wide(A)
    lam = np.sort(np.einsum('ik,ik->k', U[:2 * m, :2 * m], A.dot(U[:2 * m, :2 * m])))
    ref = np.sort(np.tile(np.linalg.eigvalsh(blk), m))
    assert conv and np.max(np.abs(lam - ref)) <= 1e-13 * np.linalg.norm(A) and np.max(np.abs(U.T.dot(U) - np.eye(U.shape[0]))) <= 1e-14


# ------------------------------------------------------------------ the facade on a recording stand-in
class FakeEngine(object):
    def __init__(self, form, device=0):
        self.n, self.calls = form.n, []

    def _answer(self, name, P0s, max_sweeps, tol):
        self.calls.append((name, max_sweeps, tol))
        B = P0s.shape[0]
        return dict(x=np.arange(B * self.n, dtype=np.float64).reshape(B, self.n), bound=10.0 + np.arange(B), mu=np.full(B, 0.5),
                    lam=np.tile(np.arange(self.n, dtype=np.float64) - 2.0, (B, 1)), sweeps=np.full(B, 11, dtype=np.int64),
                    branch=np.ones(B, dtype=np.int32), status=np.zeros(B, dtype=np.int32))

    def spectral_small_batch(self, P0s, q0s, r0s, agg, relop, max_sweeps=30, tol=1e-15):
        return self._answer('spectral_small_batch', P0s, max_sweeps, tol)

    def spectral_batch(self, P0s, q0s, r0s, agg, relop, max_sweeps=30, tol=1e-15):
        return self._answer('spectral_batch', P0s, max_sweeps, tol)


@pytest.fixture
def fake(monkeypatch):
    from qcqp_amd import batch
    monkeypatch.setattr(batch, 'Engine', FakeEngine)
    return batch


def test_facade_chooses_the_entry_point(fake):
    from qcqp_amd import problems, settings as s
    big = fake.QCQPBatch(problems.boolean_least_squares_batch(2, 65, 67, seed=1))
    with pytest.raises(Exception) as ex:
        big.suggest(s.SPECTRAL)
    msg = str(ex.value)
    assert 'QCQPBatch.suggest(SPECTRAL) is defined for n <= 64 (n = 65)' in msg and 'wide=True' in msg and big.engine.calls == []
    assert big.spectral_bound is None and big._suggested is None
    big.suggest(s.SPECTRAL, wide=True, jacobi_sweeps=20, jacobi_tol=1e-14)
    assert big.engine.calls == [('spectral_batch', 20, 1e-14)]
    assert big.spectral_sol.shape == (2, 65) and np.array_equal(big.spectral_bound, [10.0, 11.0]) and big._starts.shape == (2, 1, 65)
    assert set(big.spectral_info) == {'mu', 'lam_min', 'sweeps', 'branch', 'status'}
    with pytest.raises(Exception) as ex:
        big.suggest(s.SPECTRAL, wide=True, num_samples=2)
    assert 'num_samples must be 1' in str(ex.value)
    small = fake.QCQPBatch(problems.boolean_least_squares_batch(2, 64, 67, seed=1))
    small.suggest(s.SPECTRAL, wide=True)      # n <= 64 runs as without the keyword
    small.suggest(s.SPECTRAL)
    assert [c[0] for c in small.engine.calls] == ['spectral_small_batch', 'spectral_small_batch']


# ------------------------------------------------------------------ the rotation on the host
@pytest.fixture(scope='module')
def cxx():
    c = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++')
    if not c:
        pytest.skip('no host compiler')
    return c


def _selftest(cxx, tmp_path, extra=()):
    exe = str(tmp_path / 'spectral_wide_selftest')
    p = subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I' + os.path.join(REPO, 'tests', 'host', 'hip_stub'),
                        '-I' + os.path.join(REPO, 'qcqp_amd', 'csrc'), '-o', exe, os.path.join(REPO, 'tests', 'host', 'spectral_wide_selftest.cpp')]
                       + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode().strip()
    assert r.returncode == 0 and out.startswith('ok '), out
    return int(out.split()[1])


def test_rotation_against_long_double(cxx, tmp_path):
    assert _selftest(cxx, tmp_path) >= 500000


def test_rotation_under_sanitizers(cxx, tmp_path):
    """The same stand-alone program under AddressSanitizer + UBSan (host code only; nothing is loaded into Python)."""
    assert _selftest(cxx, tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']) >= 500000
