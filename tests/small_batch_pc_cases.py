"""What tests/test_small_batch_pc_cpu.py and tests/test_gpu_small_batch_pc.py share: the families of
problems.per_problem_constraints_batch, the coefficient array cons (B, m, 3) rebuilt from the problems' functions independently of
qcqp_amd.batch, and the cases of the SDR test.  A plain module, not a conftest: the test files import what they use."""
import itertools

import numpy as np

FAMILIES = ('boxpp', 'boxppneg', 'eq2pp', 'eqpp', 'annpp', 'linpp')
MAXC4 = ('annpp', 'linpp')                       # two constraints on a coordinate: the <4,pc> kernel
SDR_NS, SDR_BS = (1, 7, 32, 33, 64), (1, 3, 64)


def family(name, n, B, seed=1):
    from qcqp_amd import problems
    return problems.per_problem_constraints_batch(name, n, [seed + b for b in range(B)])


def entry(P, q):
    """The coordinate a separable constraint touches, its diagonal entry and its linear entry."""
    Pd = np.asarray(P.toarray() if hasattr(P, 'toarray') else P, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).ravel()
    touched = sorted(set(np.nonzero(np.diag(Pd))[0]) | set(np.nonzero(q)[0]))
    assert len(touched) == 1 and np.count_nonzero(Pd) <= 1
    i = int(touched[0])
    return i, Pd[i, i], q[i]


def cons_of(fl):
    """cons (B, m, 3): (p, q, r) of constraint k of problem b, in constraint order."""
    out = np.empty((len(fl), len(fl[0]) - 1, 3))
    for b, funcs in enumerate(fl):
        for k, (P, q, r, _) in enumerate(funcs[1:]):
            _, out[b, k, 0], out[b, k, 1] = entry(P, q)
            out[b, k, 2] = float(r)
    return out


def sdr_cases():
    """(n, B, problem seeds, seed, seed_stride, first_index) of the SDR test: every n with every B.  The problem seeds, the seed and
    the stride depend on n alone, so the batches of 1 and 3 are the first problems of the batch of 64 -- the same problems from the
    same keyed starts: the NumPy restatement of the CPU test runs the 64 and has run them all."""
    return [(n, B, [40 + 100 * j + b for b in range(B)], 23 + j, 3, 5 * j)
            for (j, n), B in itertools.product(enumerate(SDR_NS), SDR_BS)]
