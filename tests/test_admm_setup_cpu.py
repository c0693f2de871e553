"""The device-side setup of batched ADMM (qcqpmi_admm_batch_setup, Engine.admm_batch_setup, QCQPBatch.improve(ADMM, setup='device'))
without a GPU: the symbol is declared, bound and exported within ABI 6 and the new headers reach the units that build them; the LDS
figures; the cases of the grid and the padding rule on the NumPy restatement of the two setup kernels (tests/admm_setup_cases.py); a
given rho; the facade's keyword on a recording stand-in.  On the commit before the feature the symbol, the method and the keyword are
missing.  The restatement over the WHOLE grid against the oracle and eigvalsh, and the host program for csrc/admm_setup_rule.h, are
in tests/test_setup_grid_cpu.py: they take 20 s, and this file is collected before tests/test_host_cpu.py, whose rendezvous test
asserts that the test process is younger than dist.RANK_START_WINDOW (300 s) -- the files collected before it take most of that."""
import os
import re

import numpy as np
import pytest

import admm_setup_cases as asc
from conftest import REPO

SYMBOL = 'qcqpmi_admm_batch_setup'


def test_symbol_in_header_binding_library_and_build_units():
    with open(os.path.join(REPO, 'include', 'qcqp_mi.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+%s\s*\(' % SYMBOL, header)
    assert re.search(r'#define\s+QCQPMI_ABI_VERSION\s+6\b', header)
    from qcqp_amd import _build, _ffi
    proto = {p[0]: p for p in _ffi.PROTOTYPES}
    assert len(proto[SYMBOL][2]) == 11
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL) and lib.qcqpmi_abi_version() == 6
    # the kernels are built in the unit of the eigen-solvers; the driver sees the launcher's declarations only
    reach = {h: sorted(u for u in _build.TRANSLATION_UNITS if os.path.join(_build.SRC, h) in _build.unit_sources(u))
             for h in ('admm_setup.h', 'admm_setup_kernel.h', 'admm_setup_rule.h')}
    assert reach['admm_setup.h'] == ['capi_small.hip', 'spectral_small.hip']
    assert reach['admm_setup_kernel.h'] == ['spectral_small.hip'] and reach['admm_setup_rule.h'] == ['spectral_small.hip']
    text = {h: open(os.path.join(_build.SRC, h)).read() for h in reach}
    assert '__global__' not in text['admm_setup.h'] and '__global__' not in text['admm_setup_rule.h']
    assert text['admm_setup_kernel.h'].count('__global__') == 2
    # the kernel header includes what it uses and nothing else: every header it names contributes a name to its text
    uses = {'admm_setup.h': 'AdmmSetupArgs', 'admm_setup_rule.h': 'admm_setup_weight', 'dev_util.h': 'wave_max', 'jacobi_small.h': 'jacobi_small(',
            'jacobi_wide.h': 'jacobi_wide('}
    assert sorted(re.findall(r'#include "([^"]+)"', text['admm_setup_kernel.h'])) == sorted(uses)
    body = text['admm_setup_kernel.h'].split('namespace qcqpmi {', 1)[1]
    for h, word in uses.items():
        assert word in body, (h, word)
    assert re.findall(r'#include "([^"]+)"', text['admm_setup.h']) == [] and re.findall(r'#include "([^"]+)"', text['admm_setup_rule.h']) == []
    assert lib.qcqpmi_admm_batch_setup(None, 1, None, None, 30, 1e-15, None, None, None, None, None) == -1


def test_lds_of_the_setup_kernels():
    """Narrow: A, Q, the rotations of a round and w.  Wide: G, two row buffers and w -- within what spectral_wide_kernel takes."""
    n2 = lambda n: (n + 1) & ~1
    narrow = lambda n: (2 * 65 * n2(n) + 96 + 64) * 8
    wide = lambda n: (n2(n) * (n2(n) + 1) + 3 * 128) * 8
    assert narrow(64) == 67840 and 160 * 1024 // narrow(64) == 2 and 160 * 1024 // narrow(32) == 4
    assert wide(128) == 135168 and wide(128) <= 137216 and 160 * 1024 // wide(65) == 4
    with open(os.path.join(REPO, 'qcqp_amd', 'csrc', 'admm_setup.h')) as f:
        text = f.read()
    assert '67 840' in text and '135 168' in text


# ------------------------------------------------------------------ the restatement (its grid: tests/test_setup_grid_cpu.py)
def test_cases_cover_both_kernels_and_both_branches():
    cs = asc.cases()
    assert len(cs) == len(set(cs)) == 6 * 14 * 2
    assert {c[1] for c in cs if c[1] <= 64} == set(asc.SIZES) and {c[1] for c in cs if c[1] > 64} == set(asc.SIZES_WIDE)
    assert asc.restated('bls', 33, 0)['lambda_min'] > 0 > asc.restated('cut', 33, 0)['lambda_min']
    d = np.diag(asc.problem('diag', 33, 0)[1])
    assert d.min() < 0 < d.max() and np.count_nonzero(asc.problem('diag', 33, 0)[1]) == 33
    assert asc.LMIN_BOUND == 10.0 * asc.LMIN_MEASURED


def test_padding_index_enters_neither_the_minimum_nor_the_sums():
    """An odd n with lambda_min > 0: the padding coordinate's eigenvalue 0 (narrow) / unit column (wide) would lower the minimum to 0
    -- the same branch of the rule, but a different reported lambda_min -- and add 1 / (2 rho m) to nothing inside the n x n block."""
    for n in (3, 33, 65):
        r = asc.restated('bls', n, 0)
        assert r['lambda_min'] > 1e-3 and r['U'].shape == (n, n) and r['lam'].shape == (n,)
        assert np.max(np.abs(r['U'].T.dot(r['U']) - np.eye(n))) <= 1e-14


def test_given_rho():
    fl, P0s, m, rho_ok, rho_small, lmin = asc.given_rho_case()
    from qcqp_amd import batch
    short = lmin + m * rho_small < 0
    assert short.any() and not short.all()
    for b in range(3):
        r = asc.restate(P0s[b], m, rho=rho_ok)
        assert r['status'] == 0 and r['rho'] == rho_ok and np.array_equal(r['Minv'], r['Minv'].T)
        assert np.max(np.abs(r['Minv'] - batch.admm_minvs(P0s[b:b + 1], [rho_ok], m)[0])) <= 1e-12 * np.max(np.abs(r['Minv']))
        r = asc.restate(P0s[b], m, rho=rho_small)
        assert r['status'] == (3 if short[b] else 0) and r['rho'] == rho_small and (r['Minv'] is None) == bool(short[b])


# ------------------------------------------------------------------ the facade on a recording stand-in
class FakeEngine(object):
    """Answers admm_batch_setup from the restatement (or with the statuses it is told to) and records what the run is given."""
    status_override = None

    def __init__(self, form, device=0):
        self.n, self.m, self.calls = form.n, form.m, []

    def admm_batch_setup(self, P0s, rho=None, max_sweeps=30, tol=1e-15):
        self.calls.append(('admm_batch_setup', rho))
        rs = [asc.restate(P, self.m, rho=rho, max_sweeps=max_sweeps, tol=tol) for P in P0s]
        out = dict(rho=np.array([r['rho'] for r in rs]), lambda_min=np.array([r['lambda_min'] for r in rs]),
                   Minv=np.stack([r['Minv'] if r['Minv'] is not None else np.zeros((self.n, self.n)) for r in rs]),
                   sweeps=np.array([r['sweeps'] for r in rs], dtype=np.int64), status=np.array([r['status'] for r in rs], dtype=np.int32))
        if self.status_override is not None:
            out['status'] = np.array(self.status_override, dtype=np.int32)
        return out

    def _run(self, name, P0s, R, rhos, Minvs):
        self.calls.append((name, np.array(rhos), np.array(Minvs)))
        B = P0s.shape[0]
        return dict(iters1=np.ones((B, R), dtype=np.int64), iters2=np.ones((B, R), dtype=np.int64), f0=np.zeros((B, R)), maxviol=np.zeros((B, R)),
                    X=None, best_index=np.zeros(B, dtype=np.int64), best_f0=np.zeros(B), best_maxviol=np.zeros(B), best_x=np.zeros((B, self.n)))

    def admm_small_batch_run(self, P0s, q0s, r0s, R, rhos, Minvs, **kw):
        return self._run('admm_small_batch_run', P0s, R, rhos, Minvs)

    def admm_batch_run(self, P0s, q0s, r0s, R, rhos, Minvs, **kw):
        return self._run('admm_batch_run', P0s, R, rhos, Minvs)

    def cd_small_batch_run(self, P0s, q0s, r0s, R, **kw):
        self.calls.append(('cd_small_batch_run',))
        B = P0s.shape[0]
        return dict(self._run('cd', P0s, R, [], []), status1=np.zeros((B, R), dtype=np.int32), status2=np.zeros((B, R), dtype=np.int32))

    def last_admm_kernel(self):
        return 'fake', 0

    def last_cd_kernel(self):
        return 'fake'


@pytest.fixture
def fake(monkeypatch):
    from qcqp_amd import batch
    monkeypatch.setattr(batch, 'Engine', FakeEngine)
    monkeypatch.setattr(FakeEngine, 'status_override', None)
    return batch


def test_facade_keyword(fake):
    from qcqp_amd import settings as s
    fl = asc.ab.family('bls', 33, 3, seed=4)
    qb = fake.QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=5, seed=3)
    with pytest.raises(Exception, match="setup must be 'host' or 'device'"):
        qb.improve(s.ADMM, num_iters=5, setup='gpu')
    assert qb.engine.calls == []                                            # before any launch
    qb.improve(s.ADMM, num_iters=5)                                         # the default is the host path, untouched
    assert [c[0] for c in qb.engine.calls] == ['admm_small_batch_run']
    host_rho, host_minv = qb.engine.calls[0][1], qb.engine.calls[0][2]
    assert np.array_equal(host_rho, fake.admm_rhos(qb.P0s, 33)) and np.array_equal(host_minv, fake.admm_minvs(qb.P0s, host_rho, 33))
    assert qb.last_stats['setup'] == 'host' and qb.last_stats['lambda_min'] is None and qb.last_stats['setup_sweeps'] is None
    del qb.engine.calls[:]
    qb.improve(s.ADMM, num_iters=5, setup='device')
    assert [c[0] for c in qb.engine.calls] == ['admm_batch_setup', 'admm_small_batch_run'] and qb.engine.calls[0][1] is None
    dev_rho, dev_minv = qb.engine.calls[1][1], qb.engine.calls[1][2]
    assert np.max(np.abs(dev_rho - host_rho) / host_rho) <= 1e-12 and np.max(np.abs(dev_minv - host_minv)) <= 1e-12 * np.max(np.abs(host_minv))
    assert qb.last_stats['setup'] == 'device' and qb.last_stats['lambda_min'].shape == (3,) and qb.last_stats['setup_sweeps'].shape == (3,)
    assert np.array_equal(qb.last_stats['rho'], dev_rho)
    del qb.engine.calls[:]
    qb.improve(s.COORD_DESCENT, num_iters=5, setup='anything')              # COORD_DESCENT ignores the keyword
    assert qb.engine.calls[0] == ('cd_small_batch_run',)
    # an inverse from a decomposition that cannot be trusted is not used: the first such problem is named, nothing is launched after
    for status, word in (([0, 1, 1], 'problem 1 did not converge'), ([0, 0, 2], 'problem 2 is not finite')):
        FakeEngine.status_override = status
        del qb.engine.calls[:]
        with pytest.raises(Exception, match=word):
            qb.improve(s.ADMM, num_iters=5, setup='device')
        assert [c[0] for c in qb.engine.calls] == ['admm_batch_setup']
    FakeEngine.status_override = None
    # setup='device' does not admit n > 64 by itself
    big = fake.QCQPBatch(asc.ab.family('bls', 65, 2, seed=4))
    big.suggest(s.RANDOM, num_samples=2, seed=3)
    with pytest.raises(Exception, match='wide=True'):
        big.improve(s.ADMM, num_iters=5, setup='device')
    assert big.engine.calls == []
    big.improve(s.ADMM, num_iters=5, setup='device', wide=True)
    assert [c[0] for c in big.engine.calls] == ['admm_batch_setup', 'admm_batch_run']


def test_facade_words_a_small_rho_as_the_host_path_does(fake):
    from qcqp_amd import settings as s
    fl, P0s, m, rho_ok, rho_small, lmin = asc.given_rho_case()
    with pytest.raises(Exception) as host:
        fake.admm_rhos(P0s, m, rho_small)
    first_bad = int(np.nonzero(lmin + m * rho_small < 0)[0][0])
    assert re.match(r'rho parameter is too small, need at least .*problem %d' % first_bad, str(host.value))
    qb = fake.QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=2, seed=3)
    with pytest.raises(Exception) as dev:
        qb.improve(s.ADMM, num_iters=5, rho=rho_small, setup='device')
    assert str(dev.value) == str(host.value)
    assert [c[0] for c in qb.engine.calls] == ['admm_batch_setup']          # before any ADMM launch
    qb.improve(s.ADMM, num_iters=5, rho=rho_ok, setup='device')
    assert np.array_equal(qb.engine.calls[-1][1], np.full(3, rho_ok)) and qb.engine.calls[-2] == ('admm_batch_setup', rho_ok)
