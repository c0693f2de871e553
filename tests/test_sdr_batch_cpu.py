"""The batched SDR suggest (qcqpmi_sdr_small_batch, QCQPBatch.suggest(SDR)) without a GPU: the symbol is declared, bound and
exported and the ABI version did not move; the projector factor F = diag(s) V_n (I - u u^T) reproduces Sigma; certify_batch equals
dual_certificate + certify problem by problem; and the yardstick of tests/test_gpu_sdr_batch.py: a NumPy restatement of the mixing
method run on EXACTLY that file's grid (families, sizes, seeds, the documented keyed start, tol = 1e-13, max_sweeps = 20000) certifies
every problem with a margin of at least ten times the project's threshold lambda_min >= -1e-6 (1 + max |C|) and stays under the sweep
limit -- so the GPU file may assert the threshold itself.  Measured on the 24 cases (483 problems): worst lambda_min / scale
-8.6e-08, most sweeps 12870; about TWO MINUTES of `pytest -m "not gpu"` on 8 cores
(the sizes run side by side, a size's families stacked into one run).  On the commit before the feature the symbol test and the
certify_batch test fail (symbol, translation unit and function are missing); the projector identity and the grid restatement are
yardsticks in NumPy alone and pass there too."""
import os
import re

import numpy as np
import pytest

import sdr_batch_cases as sc
from conftest import REPO, oracle_map

SYMBOL = 'qcqpmi_sdr_small_batch'


def test_symbol_in_header_binding_and_library():
    with open(os.path.join(REPO, 'include', 'qcqp_mi.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+%s\s*\(' % SYMBOL, header)
    assert re.search(r'#define\s+QCQPMI_ABI_VERSION\s+6\b', header)
    from qcqp_amd import _ffi
    proto = [p for p in _ffi.PROTOTYPES if p[0] == SYMBOL]
    assert len(proto) == 1 and len(proto[0][2]) == 17
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL) and lib.qcqpmi_abi_version() == 6
    from qcqp_amd import _build
    assert 'sdr_small.hip' in _build.TRANSLATION_UNITS
    assert os.path.exists(os.path.join(_build.SRC, 'sdr_small.hip')) and os.path.exists(os.path.join(_build.SRC, 'sdr_small.h'))
    import qcqp_amd
    assert 'QCQPBatch' not in qcqp_amd.__all__ and len(qcqp_amd.__all__) == 8


def test_projector_factor_reproduces_sigma():
    """F = diag(s) V_n (I - u u^T): F F^T = diag(s) (V_n V_n^T - (V_n u)(V_n u)^T) diag(s) = Sigma of qcqp.py:395 with X = V V^T."""
    rs = np.random.RandomState(3)
    for n in (1, 2, 7, 33, 64):
        V = rs.randn(n + 1, sc.K)
        V /= np.linalg.norm(V, axis=1)[:, None]
        s = np.sqrt(rs.uniform(0.25, 4.0, size=n))
        Vn, u = V[:n], V[n]
        F = s[:, None] * (Vn - np.outer(Vn.dot(u), u))
        mu = Vn.dot(u)
        Sigma = np.outer(s, s) * (Vn.dot(Vn.T) - np.outer(mu, mu))
        assert np.max(np.abs(F.dot(F.T) - Sigma)) <= 1e-13, n
        # ... and the lifted solution in the original variables has exactly this mean and covariance
        X = V.dot(V.T) * np.outer(np.append(s, 1.0), np.append(s, 1.0))
        assert np.max(np.abs(X[:-1, -1] - s * mu)) <= 1e-13 and np.max(np.abs(X[:-1, :-1] - np.outer(X[:-1, -1], X[:-1, -1]) - Sigma)) <= 1e-13, n


def test_certify_batch_equals_the_single_problem_certificate(caplog):
    from qcqp_amd import sdr
    from qcqp_amd.form import QCQPForm
    fl = sc.family('scaled', 7, 3, seed=2)
    P0s, q0s, r0s = sc.objectives(fl)
    d = sc.d_of(fl[0])
    C = sdr.lifted_cost_batch(P0s, q0s, r0s, d)
    assert np.array_equal(C, sc.lifted(P0s, q0s, r0s, d))
    for b in range(3):
        form = QCQPForm.from_arrays(fl[b])
        assert np.array_equal(sdr.unit_diagonal_family(form), d)
        assert np.array_equal(sdr.lifted_cost(form, d)[0], C[b])
    rs = np.random.RandomState(0)
    V0 = rs.randn(3, 8, sc.K)
    V0 /= np.linalg.norm(V0, axis=2)[:, :, None]
    V, sweeps = sc.mixing_numpy(C, V0, tol=1e-13, max_sweeps=5000)
    y = np.stack([sdr.dual_certificate(C[b], V[b])[0] for b in range(3)])
    cert = sdr.certify_batch(C, y, sweeps, 5000)
    for b in range(3):
        yb, lmin, lower = sdr.dual_certificate(C[b], V[b])
        assert abs(cert['lambda_min'][b] - lmin) <= 1e-12 * cert['scale'][b] and abs(cert['bound'][b] - lower) <= 1e-9 * (1 + abs(lower))
        assert cert['converged'][b] and cert['scale'][b] == 1.0 + np.max(np.abs(C[b]))
    # the sweep limit alone withdraws the certificate (a warning, as certify logs one); a slack far from PSD raises (as certify does)
    with caplog.at_level('WARNING', logger='qcqp_amd'):
        lim = sdr.certify_batch(C, y, np.array([5000, 10, 10]), 5000)
    assert list(lim['converged']) == [False, True, True] and 'not solved to optimality' in caplog.text
    with pytest.raises(Exception) as ex:
        sdr.certify_batch(C, y - cert['scale'][:, None], sweeps, 5000)
    assert 'Relaxation problem status' in str(ex.value)


def _solve_size(orc, cases):
    """The cases of ONE n stacked into one run of the restatement (a problem does not see its neighbours): per case the worst
    lambda_min / (1 + max |C|) and the most sweeps."""
    Cs, V0s = [], []
    for name, n, B, S, pseed, seed, stride, fi in cases:
        fl = sc.family(name, n, B, seed=pseed)
        P0s, q0s, r0s = sc.objectives(fl)
        Cs.append(sc.lifted(P0s, q0s, r0s, sc.d_of(fl[0])))
        V0s.append(sc.keyed_starts(orc, B, n + 1, seed, stride))
    C = np.concatenate(Cs)
    V, sweeps = sc.mixing_numpy(C, np.concatenate(V0s))
    out, lo = [], 0
    for case in cases:
        hi = lo + case[2]
        worst = min(sc.certificate(C[b], V[b])[1] / (1.0 + np.max(np.abs(C[b]))) for b in range(lo, hi))
        out.append((case, worst, int(sweeps[lo:hi].max())))
        lo = hi
    return out


def test_numpy_mixing_certifies_the_gpu_grid_with_a_tenfold_margin(orc):
    cases = sc.cases()
    assert len(cases) == 24 and sorted(set(c[2:4] for c in cases)) == sorted(sc.BS)
    for name in sc.FAMILIES:        # every family meets every B and every S
        mine = [c for c in cases if c[0] == name]
        assert set(c[2] for c in mine) == {1, 3, 64} and set(c[3] for c in mine) == {1, 17, 64}
    res = sum(oracle_map(lambda n: _solve_size(orc, [c for c in cases if c[1] == n]), sorted(sc.NS, reverse=True)), [])
    assert len(res) == 24
    print('worst lambda_min / scale %.3e, most sweeps %d' % (min(r[1] for r in res), max(r[2] for r in res)))
    for case, worst, most in res:
        assert worst >= -1e-7, (case, worst)            # ten times inside -1e-6 (1 + max |C|)
        assert most < sc.MAX_SWEEPS, (case, most)
