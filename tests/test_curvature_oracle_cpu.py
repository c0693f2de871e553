"""The fast separable oracle (Problem.improve_cd_sep) against the restatement pinned to the reference (Problem.improve_cd) on
problems.box_qp -- the box-constrained QP with an indefinite objective, whose diagonal has positive, negative and (optionally) zero
entries -- by the rule tests/test_oracle_golden.py uses for the other families: every counter equal, points within 1e-12.  The GPU
tests of the mixed-sign step kind (tests/test_gpu_life_curvature.py) compare cd_life_kernel with improve_cd_sep; this file is their
licence to do so.  No GPU."""
import numpy as np
import pytest

SHAPES = {
    # n, box, zero_every, density, relop, diagonal
    'mixed': dict(n=48, lo=-1.0, hi=1.0),
    'mixed_zeros_unit_box': dict(n=100, lo=0.0, hi=1.0, zero_every=5),
    'mixed_zeros_sparse': dict(n=200, lo=-1.0, hi=1.0, zero_every=7, density=0.2),
    'negative': dict(n=72, lo=-1.0, hi=1.0, diagonal='negative'),
    'two_intervals': dict(n=64, lo=-1.0, hi=1.0, zero_every=7, relop='=='),          # x_i^2 == 1
    'two_intervals_unit_box': dict(n=80, lo=0.0, hi=1.0, relop='=='),                # x_i (x_i - 1) == 0: a constraint with a linear term
}


def test_box_qp_generator():
    """The generator's contract: a symmetric P0 with the requested diagonal, q0 of scale sqrt(n), one constraint per coordinate."""
    from qcqp_amd import problems
    funcs, maxi, info = problems.box_qp(60, seed=2, lo=0.0, hi=1.0, zero_every=4, density=0.5)
    P0, q0, r0, relop = funcs[0]
    assert not maxi and relop is None and r0 == 0.0 and len(funcs) == 61
    assert np.array_equal(P0, P0.T) and np.array_equal(np.diag(P0), info['diag'])
    d = info['diag']
    assert (d[3::4] == 0.0).all() and (d > 0).any() and (d < 0).any()
    off = P0 - np.diag(d)
    assert 0.3 < (off != 0).mean() < 0.7
    for i, (P, q, r, rel) in enumerate(funcs[1:]):
        assert P.nnz == 1 and P[i, i] == 1.0 and q[i] == -1.0 and np.count_nonzero(q) == 1 and r == 0.0 and rel == '<='
    neg = problems.box_qp(40, seed=2, diagonal='negative')[2]['diag']
    assert (neg < 0).all()
    only = problems.box_qp(40, seed=2, diagonal='only')[0][0][0]
    assert np.array_equal(only, np.diag(np.diag(only)))


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_sep_oracle_equals_restatement_on_box_qp(orc, shape):
    """Eight keyed restarts to convergence: the two oracles' phase-1 and phase-2 counters are equal and their points agree to 1e-12."""
    from qcqp_amd import problems
    kw = SHAPES[shape]
    funcs, _, info = problems.box_qp(seed=3, **kw)
    d = info['diag']
    if kw.get('diagonal') != 'negative':
        assert (d > 0).any() and (d < 0).any() and ((d == 0).any() == bool(kw.get('zero_every')))
    prob = orc.Problem(funcs)
    moved = 0
    for k in range(8):
        x0 = np.random.RandomState(100 + k).randn(kw['n'])
        outs = []
        for fn in (prob.improve_cd_sep, prob.improve_cd):
            rng = orc.Rng(orc.RNG_KEYED, 11)
            rng.set_restart(5 + k)
            outs.append(fn(x0, num_iters=1000, rng=rng))
        (xa, a1, a2), (xb, b1, b2) = outs
        assert tuple(a1) == tuple(b1) and tuple(a2) == tuple(b2), (shape, k, tuple(a1), tuple(b1), tuple(a2), tuple(b2))
        assert np.max(np.abs(xa - xb)) <= 1e-12, (shape, k, np.max(np.abs(xa - xb)))
        moved += int(a2[2])
    assert moved > 0, 'no restart moved in phase 2'
