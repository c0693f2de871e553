"""Helpers that check lifecycle launches (qcqpmi_cd_stream_run) restart by restart against the fast separable oracle
(Problem.improve_cd_sep, pinned to the restatement by tests/test_oracle_golden.py): the starts of a population, the oracle's runs
on them, the per-restart comparison, the winner the selection rule picks, and f0 in extended precision.  A plain module, not a
conftest: the GPU test files import what they use."""
import numpy as np

from conftest import oracle_map


def make(eng_mod, funcs):
    from qcqp_amd.form import QCQPForm
    return eng_mod.Engine(QCQPForm.from_arrays(funcs))


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / (1.0 + np.abs(np.asarray(b))))


def oracle_runs(orc, prob, jobs, iters, phase1=True):
    """jobs: (x0, seed, global restart index) -> (x, stats1, stats2, f0(x), max violation(x)) of the oracle, to convergence."""
    def run(job):
        x0, sd, gidx = job
        rng = orc.Rng(orc.RNG_KEYED, sd)
        rng.set_restart(gidx)
        x, s1, s2 = prob.improve_cd_sep(x0, num_iters=iters, phase1=phase1, rng=rng)
        return x, s1, s2, prob.eval(0, x), prob.max_violation(x)
    return oracle_map(run, jobs)


class ExactObjective(object):
    """f0 of the stored problem in extended precision (long double products and sums).  The no-ridge box / disc objectives past
    n = 2304 end near 1e-5 from terms of 1e5 .. 1e6 (|Ax - b|^2 of a rank-deficient A nearly vanishes): there the reference's own
    double evaluation -- the oracle's -- is 1e-9 off the exact value as often as the kernel's sum through L is, so the objective
    is judged against this one wherever the oracle's double value and the kernel's are more than 1e-9 apart."""
    def __init__(self, funcs):
        self.funcs = funcs
        self.P = None
        self.q = np.asarray(funcs[0][1], dtype=np.longdouble).ravel()
        self.r = np.longdouble(funcs[0][2])

    def __call__(self, x):
        if self.P is None:
            P0 = self.funcs[0][0]
            self.P = np.asarray(P0.toarray() if hasattr(P0, 'toarray') else P0, dtype=np.longdouble)
        xl = np.asarray(x, dtype=np.longdouble)
        return float(xl.dot(self.P.dot(xl)) + self.q.dot(xl) + self.r)


def check_restart(o, X, k, res, iters, tag, exact=None):
    x, s1, s2, f_or, v_or = res
    assert rel(X[:, k], x) < 1e-9, (tag, k, np.max(np.abs(X[:, k] - x)))
    assert o['sweeps1'][k] == s1[0] or (s1[0] == iters and not o['ran_phase2'][k]), (tag, k, o['sweeps1'][k], s1)
    assert bool(o['ran_phase2'][k]) == (s2[0] > 0), (tag, k)
    assert o['visits2'][k] == s2[1] and o['accepted2'][k] == s2[2], (tag, k, o['visits2'][k], o['accepted2'][k], s2)
    assert o['status1'][k] == 0 and o['status2'][k] == 0, (tag, k)        # the oracle raised on none of them
    if abs(o['f0'][k] - f_or) > 1e-9 * (1 + abs(f_or)) and exact is not None:
        f_or = exact(x)
    assert abs(o['f0'][k] - f_or) <= 1e-9 * (1 + abs(f_or)) and abs(o['maxviol'][k] - v_or) <= 1e-12, (tag, k, o['f0'][k], f_or)


def oracle_winner(results):
    from qcqp_amd import dist
    return dist.select_best_host(np.array([r[3] for r in results]), np.array([r[4] for r in results]), 1e-4)[2]


def starts(eng_mod, funcs, R, sd, fi):
    e = make(eng_mod, funcs)
    e.randn(R, seed=sd, first_index=fi)
    X0 = e.download()
    e.close()
    return X0
