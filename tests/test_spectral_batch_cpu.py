"""The batched spectral suggest (qcqpmi_spectral_small_batch, QCQPBatch.suggest(SPECTRAL)) without a GPU: the symbol is declared, bound
and exported within ABI 6; the independent solver of tests/spectral_batch_cases.py bounds the brute-force optimum over {+-1}^n from
below and equals a dense search of the circle; the NumPy restatement of the kernel agrees with the independent solver on every case
of the GPU test; QCQPBatch aggregates, refuses and publishes on a fake engine; and tests/host/spectral_selftest.cpp holds the scalar
pieces of csrc/spectral_solve.h against long-double references (host compiler, -ffp-contract=off; once more under ASan + UBSan).  On
the commit before the feature the symbol is missing and the facade refuses the method."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import spectral_batch_cases as sc
from conftest import REPO

SYMBOL = 'qcqpmi_spectral_small_batch'


def test_symbol_in_header_binding_library_and_build_units():
    with open(os.path.join(REPO, 'include', 'qcqp_mi.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+%s\s*\(' % SYMBOL, header)
    assert re.search(r'#define\s+QCQPMI_ABI_VERSION\s+6\b', header)
    from qcqp_amd import _build, _ffi
    proto = [p for p in _ffi.PROTOTYPES if p[0] == SYMBOL]
    assert len(proto) == 1 and len(proto[0][2]) == 17
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL) and lib.qcqpmi_abi_version() == 6
    assert 'spectral_small.hip' in _build.TRANSLATION_UNITS
    reach = {h: sorted(u for u in _build.TRANSLATION_UNITS if os.path.join(_build.SRC, h) in _build.unit_sources(u))
             for h in ('spectral_small.h', 'jacobi_small.h', 'spectral_solve.h')}
    assert reach['spectral_small.h'] == ['capi_small.hip', 'spectral_small.hip']
    assert reach['jacobi_small.h'] == ['spectral_small.hip'] and reach['spectral_solve.h'] == ['spectral_small.hip']
    # the eigen-solver's header stands on its own: the shared device helpers and the scalar pieces, nothing of the spectral kernel
    with open(os.path.join(_build.SRC, 'jacobi_small.h')) as f:
        assert sorted(re.findall(r'#include "([^"]+)"', f.read())) == ['dev_util.h', 'spectral_solve.h']
    with open(os.path.join(_build.SRC, 'spectral_solve.h')) as f:
        assert not re.findall(r'#include "([^"]+)"', f.read())
    assert lib.qcqpmi_spectral_small_batch(None, 1, None, None, None, None, 0, 1, 30, 1e-15, None, None, None, None, None, None, None) == -1


# ------------------------------------------------------------------ the independent solver
@pytest.mark.parametrize('n', [1, 2, 3, 7, 12])
def test_independent_bound_is_below_the_brute_force_optimum(n):
    """The sphere |x|^2 = n holds {+-1}^n, so the spectral value bounds the Boolean optimum from below -- for least squares
    objectives, indefinite ones and MAXCUT (q0 = 0: the hard case)."""
    from qcqp_amd import problems
    X = np.array(list(itertools.product((-1.0, 1.0), repeat=n)))
    agg = np.concatenate([np.ones(n), np.zeros(n), [-float(n)]])
    for seed in range(4):
        rs = np.random.RandomState(100 + seed)
        G = rs.randn(n, n)
        objs = [problems.boolean_least_squares(n, n + 3, seed=seed)[0][0], (0.5 * (G + G.T), rs.randn(n), 0.0, None),
                problems.maxcut(n, 0.5, seed=seed)[0][0]]
        for P0, q0, r0, _ in objs:
            P0, q0 = sc.dense(P0), np.asarray(q0, dtype=np.float64)
            best = float(np.min(np.einsum('ki,ij,kj->k', X, P0, X) + X.dot(q0) + r0))
            ind = sc.independent(P0, q0, r0, agg, '==')
            assert ind['bound'] <= best + 1e-9 * (1.0 + abs(best)), (n, seed, ind['bound'], best)
            assert abs(np.sum(ind['x'] ** 2) - n) <= 1e-12 * n


def test_independent_equals_a_dense_search_of_the_circle():
    """n = 2: f0 over the ellipse a_0 x_0^2 + a_1 x_1^2 + beta . x + gamma = 0 on a grid of N angles.  The nearest grid angle is within
    pi / N of the minimiser, where f0 exceeds the minimum by at most max |f''| (pi / N)^2 / 2; |f''| <= 4 rho^2 |A|_2 + 2 rho |g| in
    the variable y of the circle |y| = rho."""
    N = 400001
    th = np.linspace(0.0, 2.0 * np.pi, N)
    for seed in range(12):
        rs = np.random.RandomState(seed)
        G = rs.randn(2, 2)
        P0, q0, r0 = 0.5 * (G + G.T), rs.randn(2) * (0.0 if seed % 4 == 3 else 1.0), 0.3
        a, c = rs.uniform(0.5, 2.0, size=2), rs.uniform(-1.0, 1.0, size=2)      # a_i (x_i - c_i)^2 summed, radius^2 = 1.7
        agg = np.concatenate([a, -2.0 * a * c, [float(np.sum(a * c * c)) - 1.7]])
        ind = sc.independent(P0, q0, r0, agg, '==')
        rho = np.sqrt(1.7)
        X = c[None, :] + rho * np.stack([np.cos(th), np.sin(th)], axis=1) / np.sqrt(a)[None, :]
        grid = float(np.min(np.einsum('ki,ij,kj->k', X, P0, X) + X.dot(q0) + r0))
        A = P0 / np.outer(np.sqrt(a), np.sqrt(a))
        g = (0.5 * q0 + P0.dot(c)) / np.sqrt(a)
        slack = (4.0 * rho * rho * np.linalg.norm(A, 2) + 2.0 * rho * np.linalg.norm(g)) * (np.pi / N) ** 2 / 2.0
        assert grid - slack - 1e-12 * (1 + abs(grid)) <= ind['bound'] <= grid + 1e-12 * (1 + abs(grid)), (seed, ind['bound'], grid, slack)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', sc.FAMILIES)
def test_restatement_agrees_with_the_independent_solver(name):
    """Every case of the GPU test, B = 2: the bound to 1e-9 (1 + |f|) -- the project's parity tolerance (tests/life_oracle.py) -- and the
    eigenvalues to 1e-12 |A|_F: Jacobi's error is O(n eps |A|_F), 7e-15 |A|_F at n = 64, which leaves over 100 x margin.  The
    restatement's own point is feasible and its status 0; the families take the branch they were built for."""
    want = {'maxcut': {2}, 'ident': {2}, 'nearhard': {1}, 'bls': {1}, 'eqpp': {1}, 'box11_in': {0}, 'box01_in': {0}, 'box11_out': {1},
            'box01_out': {1}}
    for n in sc.SIZES:
        fl, P0s, q0s, r0s, aggs, relop, _ = sc.case(name, n, 2)
        for b, r in enumerate(sc.restated(name, n, 2)):
            ind = sc.independent(P0s[b], q0s[b], r0s[b], aggs[b], relop)
            assert r['status'] == 0 and r['sweeps'] <= 12, (name, n, b, r['sweeps'])
            assert abs(r['bound'] - ind['bound']) <= 1e-9 * (1.0 + abs(ind['bound'])), (name, n, b, r['bound'], ind['bound'])
            assert np.max(np.abs(r['lam'] - ind['lam'])) <= 1e-12 * np.linalg.norm(r['A']), (name, n, b)
            assert r['branch'] == ind['branch'], (name, n, b)
            if name in want:
                assert r['branch'] in want[name], (name, n, b, r['branch'])
            if name in sc.REGULAR:
                assert np.max(np.abs(r['x'] - ind['x'])) <= 1e-9 * (1.0 + np.max(np.abs(ind['x']))), (name, n, b)


# ------------------------------------------------------------------ the facade on a fake engine
class FakeEngine(object):
    """Records the calls and answers suggest(SPECTRAL) with numbers that can be recognised (no GPU here)."""
    def __init__(self, form, device=0):
        self.n, self.calls, self.args = form.n, [], None

    def spectral_small_batch(self, P0s, q0s, r0s, agg, relop, max_sweeps=30, tol=1e-15):
        self.calls.append('spectral_small_batch')
        self.args = dict(agg=np.array(agg), relop=relop, max_sweeps=max_sweeps, tol=tol)
        B = P0s.shape[0]
        status = np.zeros(B, dtype=np.int32)
        status[1::3] = 1
        status[2::3] = 2
        return dict(x=np.arange(B * self.n, dtype=np.float64).reshape(B, self.n), bound=10.0 + np.arange(B), mu=np.full(B, 0.5),
                    lam=np.tile(np.arange(self.n, dtype=np.float64) - 2.0, (B, 1)), sweeps=np.full(B, 7, dtype=np.int64),
                    branch=np.ones(B, dtype=np.int32), status=status)

    def cd_small_batch_run(self, P0s, q0s, r0s, R, X0=None, **kw):
        self.calls.append('cd_small_batch_run')
        self.X0 = X0
        B = P0s.shape[0]
        z = np.zeros((B, R))
        return dict(best_x=np.zeros((B, self.n)), best_index=np.zeros(B, dtype=np.int64), f0=z, maxviol=z, status1=z, status2=z,
                    best_f0=np.zeros(B), best_maxviol=np.zeros(B))

    def sdr_small_batch(self, *a, **kw):
        self.calls.append('sdr_small_batch')
        raise AssertionError('launched')

    def last_cd_kernel(self):
        return 'none'


@pytest.fixture
def fake(monkeypatch):
    from qcqp_amd import batch
    monkeypatch.setattr(batch, 'Engine', FakeEngine)
    return batch


@pytest.mark.parametrize('name', ['bls', 'maxcut', 'box01_indef', 'eqpp', 'boxpp'])
def test_facade_aggregates_shared_and_per_problem_coefficients(fake, name):
    from qcqp_amd import settings as s
    n, B = 5, 4
    fl, P0s, q0s, r0s, aggs, relop, shared = sc.case(name, n, B)
    qb = fake.QCQPBatch(fl)
    assert (qb.cons is None) == shared
    qb.suggest(s.SPECTRAL)
    assert qb.engine.calls == ['spectral_small_batch'] and qb.engine.args['relop'] == relop
    assert (qb.engine.args['max_sweeps'], qb.engine.args['tol']) == (30, 1e-15)
    got = qb.engine.args['agg']
    assert got.shape == ((2 * n + 1,) if shared else (B, 2 * n + 1))
    assert np.allclose(got, aggs[0] if shared else aggs, rtol=1e-15, atol=0.0)
    # what is published: NaN where status != 0, the point as the single start of improve()
    ok = np.array([True, False, False, True])
    assert np.array_equal(np.isnan(qb.spectral_bound), ~ok) and np.array_equal(qb.spectral_bound[ok], np.array([10.0, 13.0]))
    assert qb.spectral_sol.shape == (B, n) and np.array_equal(np.isnan(qb.spectral_sol).all(axis=1), ~ok)
    assert np.array_equal(qb.spectral_sol[0], np.arange(n))
    info = qb.spectral_info
    assert set(info) == {'mu', 'lam_min', 'sweeps', 'branch', 'status'} and np.array_equal(info['lam_min'], np.full(B, -2.0))
    assert np.array_equal(info['status'], [0, 1, 2, 0])
    assert qb._starts.shape == (B, 1, n) and qb._starts.flags['C_CONTIGUOUS'] and qb._suggested[0] == 1
    qb.improve(s.COORD_DESCENT)
    assert qb.engine.calls == ['spectral_small_batch', 'cd_small_batch_run'] and qb.engine.X0 is qb._starts
    qb.suggest(s.SPECTRAL, certify=True)
    cert = qb.spectral_info['certificate']
    assert set(cert) >= {'c', 'feasibility', 'stationarity', 'lambda_min'} and cert['lambda_min'].shape == (B,)
    assert ('complementarity' in cert) == (relop == '<=')
    qb.suggest(s.RANDOM, num_samples=3)      # the other methods as before: RANDOM draws inside improve()
    assert qb._starts is None and qb._suggested[0] == 3


def _quad(n, i, p, q, r, relop):
    import scipy.sparse as sp
    qv = np.zeros(n)
    qv[i] = q
    return (sp.csr_matrix(([float(p)], ([i], [i])), shape=(n, n)), qv, float(r), relop)


def test_facade_refuses_outside_the_family_before_any_launch(fake):
    from qcqp_amd import problems, settings as s
    n = 4
    obj = problems.box_qp(n, seed=1)[0][0]
    boolean = [_quad(n, i, 1.0, 0.0, -1.0, '==') for i in range(n)]

    def refused(funcs_list, *words, **kw):
        qb = fake.QCQPBatch(funcs_list)
        with pytest.raises(Exception) as ex:
            qb.suggest(s.SPECTRAL, **kw)
        msg = str(ex.value)
        assert msg.startswith('QCQPBatch.suggest(SPECTRAL)') and all(w in msg for w in words), msg
        assert qb.engine.calls == [] and qb._suggested is None and qb.spectral_bound is None
        return msg

    refused([[obj] + boolean], 'num_samples must be 1', 'num_samples = 2', num_samples=2)
    refused([[obj] + boolean[:3] + [_quad(n, 3, 1.0, 0.0, -1.0, '<=')]], 'same relop', 'constraint 3 is <=', 'constraint 0 is ==')
    refused([[obj] + boolean[:3] + [_quad(n, 3, 0.0, 1.0, -1.0, '==')]], 'a_i > 0', 'coordinate 3 has a = 0')       # linear only
    refused([[obj] + boolean[:3]], 'a_i > 0', 'coordinate 3 has a = 0')                                              # unconstrained
    refused([[obj] + boolean[:3] + [_quad(n, 3, -1.0, 0.0, 1.0, '==')]], 'a_i > 0', 'coordinate 3 has a = -1')
    refused([[obj] + [_quad(n, i, 1.0, 0.0, 1.0, '<=') for i in range(n)]], 'rho^2', '> 0', 'rho^2 = -4')
    refused([[obj]], 'no constraint')
    coupled = (np.ones((n, n)), np.zeros(n), -1.0, '==')
    refused([[obj] + boolean + [coupled]], 'separable', 'constraint 4')
    # per-problem coefficients: the message names the problem
    ok = [obj] + [_quad(n, i, 1.0, -1.0, 0.0, '<=') for i in range(n)]
    bad_a = [obj] + [_quad(n, i, 1.0, -1.0, 0.0, '<=') for i in range(3)] + [_quad(n, 3, -2.0, -1.0, 0.0, '<=')]
    msg = refused([ok, ok, bad_a], 'a_i > 0', 'coordinate 3 of problem 2 has a = -2')
    bad_rho = [obj] + [_quad(n, i, 1.0, -1.0, 5.0, '<=') for i in range(n)]
    refused([ok, bad_rho, ok], 'rho^2', 'of problem 1')
    # n > 64, in the style of the SDR refusal; suggest(SDR) keeps its own
    big = fake.QCQPBatch(problems.boolean_least_squares_batch(2, 65, 67, seed=1))
    with pytest.raises(Exception) as ex:
        big.suggest(s.SPECTRAL)
    assert 'QCQPBatch.suggest(SPECTRAL) is defined for n <= 64 (n = 65)' in str(ex.value) and big.engine.calls == []
    with pytest.raises(Exception) as ex:
        big.suggest(s.SDR, num_samples=4)
    assert 'QCQPBatch.suggest(SDR) is defined for n <= 64 (n = 65) unless wide=True' in str(ex.value)
    with pytest.raises(Exception) as ex:
        big.suggest('dccp')
    assert 'QCQPBatch.suggest is defined for the RANDOM, SDR and SPECTRAL methods' in str(ex.value)


def test_certificate_tells_a_minimiser_from_another_point():
    """sdr.certify_spectral_batch on the independent solver's answers: all conditions hold to 1e-9 of the scale; a feasible point that
    is not the minimiser fails stationarity, and a multiplier below -lambda_min fails the curvature condition."""
    from qcqp_amd import sdr
    for name in ('bls', 'maxcut', 'box01_out', 'box11_in', 'boxpp'):
        fl, P0s, q0s, r0s, aggs, relop, _ = sc.case(name, 7, 3)
        ind = [sc.independent(P0s[b], q0s[b], r0s[b], aggs[b], relop) for b in range(3)]
        x, mu = np.stack([i['x'] for i in ind]), np.array([i['mu'] for i in ind])
        scale = np.array([sc.scale_of(P0s[b], q0s[b], r0s[b], aggs[b]) for b in range(3)])
        cert = sdr.certify_spectral_batch(P0s, q0s, aggs, relop, x, mu)
        assert np.all(cert['feasibility'] <= 1e-9 * scale) and np.all(cert['stationarity'] <= 1e-9 * scale), (name, cert)
        assert np.all(cert['lambda_min'] >= -1e-9 * scale), (name, cert['lambda_min'])
        if relop == '<=':
            assert np.all(cert['mu_sign'] == 0.0) and np.all(cert['complementarity'] <= 1e-9 * scale)
        if name == 'bls':
            other = sdr.certify_spectral_batch(P0s, q0s, aggs, relop, np.ones_like(x), mu)
            assert np.all(other['feasibility'] <= 1e-12) and np.all(other['stationarity'] > 1e-3 * scale / 7 ** 2)
            low = sdr.certify_spectral_batch(P0s, q0s, aggs, relop, x, -np.linalg.eigvalsh(P0s)[:, 0] - 1.0)      # a = 1: one below -lambda_min(P0)
            assert np.allclose(low['lambda_min'], -1.0, rtol=0.0, atol=1e-9)


# ------------------------------------------------------------------ the scalar pieces on the host
@pytest.fixture(scope='module')
def cxx():
    c = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++')
    if not c:
        pytest.skip('no host compiler')
    return c


def _selftest(cxx, tmp_path, extra=()):
    exe = str(tmp_path / 'spectral_selftest')
    p = subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I' + os.path.join(REPO, 'tests', 'host', 'hip_stub'),
                        '-I' + os.path.join(REPO, 'qcqp_amd', 'csrc'), '-o', exe, os.path.join(REPO, 'tests', 'host', 'spectral_selftest.cpp')]
                       + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode().strip()
    assert r.returncode == 0 and out.startswith('ok '), out
    return int(out.split()[1])


def test_scalar_pieces_against_long_double(cxx, tmp_path):
    assert _selftest(cxx, tmp_path) >= 1000000


def test_scalar_pieces_under_sanitizers(cxx, tmp_path):
    """The same stand-alone program under AddressSanitizer + UBSan (host code only; nothing is loaded into Python)."""
    assert _selftest(cxx, tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']) >= 1000000
