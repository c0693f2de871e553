"""The small-problem batch (qcqpmi_cd_small_batch_run, qcqp_amd.batch.QCQPBatch) without a GPU: the symbol is declared, bound and
exported and the ABI version did not move; QCQPBatch refuses problems whose constraints or sizes differ; the batch generators are
deterministic; and the yardstick of tests/test_gpu_small_batch.py -- the oracle's fast separable improve_cd_sep -- equals the
restatement improve_cd on the batch families at n = 1, 2, 15, 16, 17, 33, 64 (points bit-equal or within 1e-12, equal stats), and
is not chaotic there: one ulp on x0 moves no restart by more than the tolerance of the GPU comparison.  On the commit before the
feature the symbol and the module are missing and these tests fail."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

NS = (1, 2, 15, 16, 17, 33, 64)
SYMBOL = 'qcqpmi_cd_small_batch_run'


def family(name, n, B, seed=1):
    from qcqp_amd import problems
    seeds = [seed + b for b in range(B)]
    if name == 'bls':
        return problems.boolean_least_squares_batch(B, n, n + n // 2 + 1, seed=seed)
    if name == 'box01':
        return problems.box_qp_batch(n, seeds, lo=0.0, hi=1.0)
    if name == 'box11neg':
        return problems.box_qp_batch(n, seeds, lo=-1.0, hi=1.0, diagonal='negative')
    if name == 'eq2':
        return problems.box_qp_batch(n, seeds, lo=-0.5, hi=1.0, relop='==')
    if name == 'ann2':
        return [problems.multi_class('ann2', n, seed=sd) for sd in seeds]
    if name == 'cut':
        return [problems.maxcut(n, seed=sd, weighted=True)[0] for sd in seeds]
    raise KeyError(name)


FAMILIES = ('bls', 'box01', 'box11neg', 'eq2', 'ann2', 'cut')


def test_symbol_in_header_binding_and_library():
    with open(os.path.join(REPO, 'include', 'qcqp_mi.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+%s\s*\(' % SYMBOL, header)
    assert re.search(r'#define\s+QCQPMI_ABI_VERSION\s+6\b', header)
    from qcqp_amd import _ffi
    assert SYMBOL in [p[0] for p in _ffi.PROTOTYPES]
    proto = [p for p in _ffi.PROTOTYPES if p[0] == SYMBOL][0]
    assert len(proto[2]) == 30
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL) and lib.qcqpmi_abi_version() == 6
    from qcqp_amd import _build
    assert 'cd_small.hip' in _build.TRANSLATION_UNITS


def test_batch_module_is_not_in_the_star_import():
    import qcqp_amd
    assert 'QCQPBatch' not in qcqp_amd.__all__ and len(qcqp_amd.__all__) == 8
    from qcqp_amd.batch import QCQPBatch       # noqa: F401


def test_generators_are_deterministic():
    from qcqp_amd import problems
    a = problems.boolean_least_squares_batch(5, 12, 18, seed=4)
    b = problems.boolean_least_squares_batch(5, 12, 18, seed=4)
    assert len(a) == 5 and all(len(f) == 13 for f in a)
    for fa, fb in zip(a, b):
        assert np.array_equal(fa[0][0], fb[0][0]) and np.array_equal(fa[0][1], fb[0][1]) and fa[0][2] == fb[0][2]
    one = problems.boolean_least_squares(12, 18, seed=6)[0]
    assert np.array_equal(a[2][0][0], one[0][0]) and np.array_equal(a[2][0][1], one[0][1])     # problem b = seed + b
    assert not np.array_equal(a[0][0][0], a[1][0][0])
    sh = problems.boolean_least_squares_batch(3, 12, 18, seed=4, shared_A=True)
    assert np.array_equal(sh[0][0][0], sh[2][0][0]) and not np.array_equal(sh[0][0][1], sh[2][0][1])
    bq = problems.box_qp_batch(9, [3, 4, 5], lo=0.0, hi=1.0)
    assert np.array_equal(bq[1][0][0], problems.box_qp(9, seed=4, lo=0.0, hi=1.0)[0][0][0])
    assert all(f[1:] == bq[0][1:] for f in bq)


def test_qcqpbatch_rejects_mismatched_problems(monkeypatch):
    from qcqp_amd import batch, problems
    made = []
    monkeypatch.setattr(batch, 'Engine', lambda form, device=0: made.append(form) or object())     # no GPU here
    fl = problems.boolean_least_squares_batch(4, 8, 12, seed=1)
    qb = batch.QCQPBatch(fl)
    assert qb.B == 4 and qb.n == 8 and qb.P0s.shape == (4, 8, 8) and len(made) == 1
    other = problems.box_least_squares(8, 12, seed=1)[0]
    with pytest.raises(Exception) as ex:
        batch.QCQPBatch([fl[0], fl[1], other, other])
    assert 'problem 2' in str(ex.value) and 'constraints' in str(ex.value)
    with pytest.raises(Exception) as ex:
        batch.QCQPBatch([fl[0], problems.boolean_least_squares(9, 12, seed=1)[0]])
    assert 'problem 1' in str(ex.value) and 'n = 9' in str(ex.value)
    with pytest.raises(Exception):
        qb.improve()                      # nothing suggested yet


def _runs(orc, funcs, n, R, seed, bump=None):
    prob = orc.Problem(funcs)
    out = []
    for r in range(R):
        x0 = np.array([orc.keyed_normal(seed, r, j) for j in range(n)])
        if bump is not None:
            x0 = np.nextafter(x0, bump)
        both = []
        for fn in (prob.improve_cd_sep, prob.improve_cd):
            rng = orc.Rng(orc.RNG_KEYED, seed)
            rng.set_restart(r)
            both.append(fn(x0, num_iters=200, rng=rng))
        out.append(both)
    return out


@pytest.mark.parametrize('name', FAMILIES)
def test_fast_oracle_equals_the_restatement_on_the_batch_families(orc, name):
    for n in NS:
        for b, funcs in enumerate(family(name, n, 2, seed=5)):
            for (xs, s1, s2), (xr, r1, r2) in _runs(orc, funcs, n, 3, 31 + b):
                assert np.array_equal(xs, xr) or np.max(np.abs(xs - xr) / (1 + np.abs(xr))) <= 1e-12, (name, n, b)
                assert np.array_equal(s1, r1) and np.array_equal(s2, r2), (name, n, b, s1, r1, s2, r2)


@pytest.mark.parametrize('name', FAMILIES)
def test_families_are_not_chaotic_at_small_sizes(orc, name):
    """One ulp on every coordinate of x0, oracle against oracle: the same counters and the same point to 1e-9 -- what lets the GPU
    test compare EVERY restart (a family that failed this would have to leave the GPU grid; none does)."""
    for n in NS:
        funcs = family(name, n, 1, seed=5)[0]
        base = _runs(orc, funcs, n, 4, 77)
        for bump in (np.inf, -np.inf):
            for (a, _), (c, _) in zip(base, _runs(orc, funcs, n, 4, 77, bump=bump)):
                assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2]), (name, n)
                assert np.max(np.abs(a[0] - c[0]) / (1 + np.abs(c[0]))) < 1e-9, (name, n)
