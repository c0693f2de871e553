"""The ground tests/test_gpu_admm_batch.py stands on, checked without a GPU (oracle only).

improve_admm on constraints x_i^2 == d amplifies a last-bit difference by about two per iteration, so the GPU test compares restart by
restart at admm_batch_cases.NUM_ITERS = 5 iterations per phase.  Here: at that horizon the oracle itself moves by at most 1e-11 (a
hundredth of the GPU threshold 1e-9) and keeps both iteration counts when every start is perturbed by a relative 4e-16 -- for every
(family, n, problem seed, start seed) of the GPU grid; the arguments that aim at an exit of the iteration take that exit in the oracle;
the host side of QCQPBatch.improve(ADMM) -- the rho rule and the batched inverse -- agrees with the oracle's."""
import numpy as np
import pytest

import admm_batch_cases as ab
from conftest import oracle_map


def _sensitivity(orc, fl, c):
    name, n, B, R, ps, seed, stride, fi = c
    X0 = ab.starts(orc, seed, stride, fi, B, R, n)
    Xa, a1, a2, _, _ = ab.oracle_batch(orc, oracle_map, fl, X0, num_iters=ab.NUM_ITERS)
    Xb, b1, b2, _, _ = ab.oracle_batch(orc, oracle_map, fl, ab.perturbed(X0), num_iters=ab.NUM_ITERS)
    worst = max(ab.rel(Xb[b, r], Xa[b, r]) for b in range(B) for r in range(R))
    print('\n%s: oracle moves by %.1e under a relative %.0e on the starts (%d restarts)' % (ab.case_id(c), worst, ab.EPS, B * R))
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    assert worst <= ab.SENSITIVITY, worst


@pytest.mark.parametrize('c', ab.cases(), ids=ab.case_id)
def test_oracle_is_stable_at_the_parity_horizon(orc, c):
    _sensitivity(orc, ab.family(c[0], c[1], c[2], seed=c[4]), c)


@pytest.mark.parametrize('c', ab.pc_cases(), ids=ab.case_id)
def test_oracle_is_stable_at_the_parity_horizon_per_problem_coefficients(orc, c):
    _sensitivity(orc, ab.pc_family(c[0], c[1], c[2], seed=c[4]), c)


def test_improve_admm_with_counts_is_the_oracles_improve_admm(orc):
    for name, n in (('bls', 17), ('box', 16), ('ann2', 7)):
        funcs = ab.family(name, n, 1, seed=4)[0]
        prob = orc.Problem(funcs)
        for r in range(3):
            x0 = np.random.RandomState(r).randn(n)
            x, i1, i2 = ab.improve_admm(prob, x0, num_iters=ab.NUM_ITERS)
            assert np.array_equal(x, prob.improve_admm(x0, num_iters=ab.NUM_ITERS))
            assert 0 <= i1 <= ab.NUM_ITERS and 1 <= i2 <= ab.NUM_ITERS


@pytest.mark.parametrize('e', ab.exit_cases(), ids=lambda e: e[0])
def test_exit_cases_take_their_exit_in_the_oracle(orc, e):
    label, name, n, ps, kw, want = e
    fl = ab.family(name, n, 2, seed=ps)
    if label.startswith('phase1-at-0'):
        X0 = np.stack([ab.feasible_starts(name, n, ab.EXIT_R, ps + b) for b in range(2)])
    else:
        X0 = ab.starts(orc, 31, 3, 0, 2, ab.EXIT_R, n)
    X, i1, i2, _, _ = ab.oracle_batch(orc, oracle_map, fl, X0, **kw)
    assert want(i1, i2), (i1, i2)
    if label == 'phase2-by-tol':      # the exit is the distance test, not the violation limit
        assert np.all(np.isfinite(X))
    # inside the stable horizon: the counts survive the perturbation
    Xb, b1, b2, _, _ = ab.oracle_batch(orc, oracle_map, fl, ab.perturbed(X0), **kw)
    assert np.array_equal(i1, b1) and np.array_equal(i2, b2)
    assert max(ab.rel(Xb[b, r], X[b, r]) for b in range(2) for r in range(ab.EXIT_R)) <= ab.SENSITIVITY


@pytest.mark.parametrize('n,seed', ab.WINNER_CASES)
def test_winning_start_wins_both_comparisons_in_the_oracle(orc, n, seed):
    funcs, x0 = ab.winning_start(orc, n, seed)
    prob = orc.Problem(funcs)
    assert 0.0 < prob.max_violation(x0) < 1e-4
    x, i1, i2 = ab.improve_admm(prob, x0, **ab.WINNER_KW)
    assert i1 > 0 and i2 > 0                  # both phases ran
    assert np.array_equal(x, x0)              # and the start is what comes back


def test_rho_rule_and_batched_inverse_agree_with_the_oracle(orc):
    from qcqp_amd import batch
    for name, n, B in (('bls', 17, 5), ('cut', 32, 4), ('box', 33, 4), ('ann2', 16, 3), ('cut', 1, 2)):
        fl = ab.family(name, n, B, seed=9)
        P0s, q0s, r0s = ab.objectives(fl)
        m = len(fl[0]) - 1
        rhos = batch.admm_rhos(P0s, m)
        Minvs = batch.admm_minvs(P0s, rhos, m)
        assert np.array_equal(Minvs, Minvs.transpose(0, 2, 1))
        rs = np.random.RandomState(n)
        for b in range(B):
            ref = orc.Problem(fl[b]).auto_rho()
            assert abs(rhos[b] - ref) <= 1e-12 * ref
            # the oracle's solve: Cholesky of 2 (P0 + rho m I), forward and back substitution
            L = np.linalg.cholesky(2.0 * (P0s[b] + ref * m * np.eye(n)))
            rhs = rs.randn(n)
            z = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
            assert ab.rel(Minvs[b].dot(rhs), z) <= 1e-12
    # a given rho: kept where it is large enough, the reference's message (with the first problem that fails) where it is not
    fl = ab.family('cut', 16, 3, seed=2)
    P0s, _, _ = ab.objectives(fl)
    lmin = np.linalg.eigvalsh(P0s)[:, 0]
    assert np.all(lmin < 0)
    ok = float(np.max(-lmin) / 16 * 1.01)
    assert np.array_equal(batch.admm_rhos(P0s, 16, ok), np.full(3, ok))
    small = float(np.sort(-lmin)[1] / 16 * 1.0001)      # enough for one problem only... or two: the first that fails is named
    first_bad = int(np.nonzero(lmin + 16 * small < 0)[0][0])
    with pytest.raises(Exception, match=r'rho parameter is too small, need at least .*problem %d' % first_bad):
        batch.admm_rhos(P0s, 16, small)
