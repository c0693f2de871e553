"""The batch for problems of 65 to 128 variables (qcqpmi_cd_batch_run, the wide kernels cd_small_kernel<MAXC[,pc],w2>) without a GPU:
the symbol is declared, bound and exported and the ABI version did not move; QCQPBatch sends n <= 64 to cd_small_batch_run and
65 <= n <= 128 to cd_batch_run, refuses n = 129 and refuses suggest(SDR) past n = 64 before anything is launched; and the yardstick
of tests/test_gpu_wide_batch.py -- the oracle's fast separable improve_cd_sep -- equals the restatement improve_cd on the eight
shared families and the six per-problem-constraint families at every n of the wide grid (points within 1e-12, equal counters, every
restart), and is not chaotic there: one ulp on x0 in either direction moves no counter and no point by 1e-9.  That is what lets the
GPU test compare EVERY restart.  On the commit before the feature the symbol is missing and the facade refuses n = 65."""
import os
import re

import numpy as np
import pytest

import small_batch_pc_cases as pc
import wide_batch_cases as wc
from conftest import REPO, oracle_map
from test_gpu_small_batch import family

SYMBOL = 'qcqpmi_cd_batch_run'


def test_symbol_in_header_binding_and_library():
    with open(os.path.join(REPO, 'include', 'qcqp_mi.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+%s\s*\(' % SYMBOL, header)
    assert re.search(r'#define\s+QCQPMI_ABI_VERSION\s+6\b', header)
    from qcqp_amd import _ffi
    proto = [p for p in _ffi.PROTOTYPES if p[0] == SYMBOL]
    twin = [p for p in _ffi.PROTOTYPES if p[0] == 'qcqpmi_cd_small_batch_run_pc'][0]
    assert len(proto) == 1 and proto[0][1:] == twin[1:] and len(proto[0][2]) == 31      # the arguments of the _pc symbol
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL) and lib.qcqpmi_abi_version() == 6


class FakeEngine(object):
    """Records which entry point the facade calls (no GPU here)."""
    def __init__(self, form, device=0):
        self.n, self.calls = form.n, []

    def _out(self, name, P0s, R):
        self.calls.append(name)
        B = P0s.shape[0]
        z = np.zeros((B, R))
        return dict(best_x=np.zeros((B, self.n)), best_index=np.zeros(B, dtype=np.int64), f0=z, maxviol=z, status1=z, status2=z,
                    best_f0=np.zeros(B), best_maxviol=np.zeros(B))

    def cd_small_batch_run(self, P0s, q0s, r0s, R, **kw):
        return self._out('cd_small_batch_run', P0s, R)

    def cd_batch_run(self, P0s, q0s, r0s, R, **kw):
        return self._out('cd_batch_run', P0s, R)

    def sdr_small_batch(self, *a, **kw):
        self.calls.append('sdr_small_batch')
        raise AssertionError('launched')

    def last_cd_kernel(self):
        return 'none'


@pytest.mark.parametrize('n,entry', [(64, 'cd_small_batch_run'), (65, 'cd_batch_run'), (128, 'cd_batch_run')])
def test_qcqpbatch_picks_the_entry_point_by_n(monkeypatch, n, entry):
    from qcqp_amd import batch, problems, settings as s
    monkeypatch.setattr(batch, 'Engine', FakeEngine)
    qb = batch.QCQPBatch(problems.boolean_least_squares_batch(2, n, n + 2, seed=1))
    qb.suggest(s.RANDOM, num_samples=3, seed=2)
    qb.improve(s.COORD_DESCENT)
    assert qb.engine.calls == [entry]
    qp = batch.QCQPBatch(problems.per_problem_constraints_batch('boxpp', n, [1, 2]))      # per-problem coefficients: the same rule
    assert qp.cons.shape == (2, n, 3)
    qp.suggest(s.RANDOM, num_samples=3, seed=2)
    qp.improve(s.COORD_DESCENT)
    assert qp.engine.calls == [entry]


def test_qcqpbatch_refuses_n_129_and_sdr_past_64(monkeypatch):
    from qcqp_amd import batch, problems, settings as s
    made = []
    monkeypatch.setattr(batch, 'Engine', lambda form, device=0: made.append(1) or FakeEngine(form))
    with pytest.raises(Exception) as ex:
        batch.QCQPBatch(problems.boolean_least_squares_batch(2, 129, 131, seed=1))
    assert 'n = 129' in str(ex.value) and '128' in str(ex.value) and not made
    qb = batch.QCQPBatch(problems.boolean_least_squares_batch(2, 65, 67, seed=1))
    with pytest.raises(Exception) as ex:
        qb.suggest(s.SDR, num_samples=4, seed=1)
    assert 'SDR' in str(ex.value) and '64' in str(ex.value) and qb.engine.calls == []      # before any launch
    ok = batch.QCQPBatch(problems.boolean_least_squares_batch(2, 64, 66, seed=1))          # n = 64 still reaches the SDR launch
    with pytest.raises(AssertionError):
        ok.suggest(s.SDR, num_samples=4, seed=1)
    assert ok.engine.calls == ['sdr_small_batch']


def _funcs(name, n, fseed):
    if name in pc.FAMILIES:
        return pc.family(name, n, 1, seed=fseed)[0]
    return family(name, n, 1, seed=fseed)[0]


def _runs(orc, funcs, n, R, seed, fns, bump=None):
    prob = orc.Problem(funcs)
    out = []
    for r in range(R):
        x0 = np.array([orc.keyed_normal(seed, r, j) for j in range(n)])
        if bump is not None:
            x0 = np.nextafter(x0, bump)
        both = []
        for fn in fns:
            rng = orc.Rng(orc.RNG_KEYED, seed)
            rng.set_restart(r)
            both.append(getattr(prob, fn)(x0, num_iters=wc.ITERS, rng=rng))
        out.append(both)
    return out


ALL = wc.SHARED + pc.FAMILIES


@pytest.mark.parametrize('name', ALL)
def test_fast_oracle_equals_the_restatement_at_the_wide_sizes(orc, name):
    def one(n):
        fseed, seed = wc.cpu_seeds(name, n)
        for (xs, s1, s2), (xr, r1, r2) in _runs(orc, _funcs(name, n, fseed), n, 4, seed, ('improve_cd_sep', 'improve_cd')):
            assert np.max(np.abs(xs - xr) / (1 + np.abs(xr))) <= 1e-12, (name, n)
            assert np.array_equal(s1, r1) and np.array_equal(s2, r2), (name, n, s1, r1, s2, r2)
    oracle_map(one, sorted(wc.NW, reverse=True))


@pytest.mark.parametrize('name', ALL)
def test_families_are_not_chaotic_at_the_wide_sizes(orc, name):
    """One ulp on every coordinate of x0, in either direction, oracle against oracle: equal counters, the point within 1e-9."""
    def one(n):
        fseed, seed = wc.cpu_seeds(name, n)
        funcs = _funcs(name, n, fseed)
        base = _runs(orc, funcs, n, 4, seed, ('improve_cd_sep',))
        for bump in (np.inf, -np.inf):
            for (a,), (c,) in zip(base, _runs(orc, funcs, n, 4, seed, ('improve_cd_sep',), bump=bump)):
                assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2]), (name, n)
                assert np.max(np.abs(a[0] - c[0]) / (1 + np.abs(c[0]))) < 1e-9, (name, n)
    oracle_map(one, sorted(wc.NW, reverse=True))
