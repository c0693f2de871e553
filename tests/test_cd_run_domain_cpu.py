"""CPU side of tests/test_gpu_cd_run_domain.py, without a GPU:
  * every case's typed-in instantiation equals what dispatch() -- the restatement of launch_cd's conditions -- derives from the
    problem's arrays, and the cells at a bound of the dispatch sit exactly there (one block of 16 away the line differs);
  * every oracle workload of the GPU file, at its actual size, seeds and starts (keyed normals from the oracle's own generator,
    which the GPU tests pin to Engine.randn): Problem.improve_cd_sep returns without an error code on every restart, converges
    below the num_iters the GPU test passes, and the workload of a case stays within a few seconds of wall time;
  * the families of the grid the fast oracle had not been pinned on (a zero diagonal with one inequality class, a diagonal of all
    three signs beside the padding class, 23 classes, two and three constraints of random kinds per coordinate on an indefinite
    objective, exact ties of a diagonal objective) against the restatement Problem.improve_cd at n = 24 / 33: equal counters, points
    within 1e-12, bit-identical where phase 2 did not run.

Measured CPU seconds of the oracle workload per case (all restarts of the case, side by side on the host's cores): see
profiles/r09_cd_run_domain.md; the largest is below 3 s, the whole file's workload below 40 s."""
import functools
import time

import numpy as np
import pytest

import test_gpu_cd_run_domain as dom
from conftest import oracle_map

BUDGET_S = 10.0        # per case, all its restarts side by side: what keeps a GPU test at a few seconds (measured: <= 3 s)


@functools.lru_cache(maxsize=None)
def problem(fam, n):
    return dom.family(fam, n)


@pytest.mark.parametrize('name', sorted(dom.CASES))
def test_typed_in_instantiation_is_what_the_dispatch_conditions_give(name):
    c = dom.CASES[name]
    s = dom.shape(problem(c['fam'], c['n']))
    assert dom.dispatch(s, c['queue'], c['dbg'], c['generic']) == c['want'], (name, s)
    assert 21 <= c['R'] <= 40 or name == 'qs-r5'
    assert c['R'] % 16 != 0 and c['first'] != 0


def _neighbour(name, step):
    c = dom.CASES[name]
    return dom.dispatch(dom.shape(problem(c['fam'], c['n'] + step)), c['queue'], c['dbg'], c['generic'])


@pytest.mark.parametrize('name,below', dom.FIRST_PAST, ids=['%s|%s' % f for f in dom.FIRST_PAST])
def test_cells_past_a_bound_are_the_first_past_it(name, below):
    assert below not in dom.CASES[name]['want'] and below in _neighbour(name, -16), (name, _neighbour(name, -16))


@pytest.mark.parametrize('name,inside', dom.LAST_INSIDE, ids=[f[0] for f in dom.LAST_INSIDE])
def test_cells_at_the_upper_edge_are_the_last_inside(name, inside):
    assert inside in dom.CASES[name]['want'] and inside not in _neighbour(name, 16), (name, _neighbour(name, 16))


def test_grid_reaches_every_reachable_instantiation():
    wants = {c['want'] for c in dom.CASES.values()}
    assert {dom.Q % cs for cs in (0, 2, 4, 6)} <= wants and {dom.QS % 0, dom.QS % 4} <= wants
    assert {dom.RS % (xl, fa, 1, sym) for xl in (0, 1) for fa in (1, 2) for sym in (0, 1)} <= wants
    assert {dom.GEN % (1, xl, 1, fa, 0) for xl in (0, 1) for fa in (0, 1, 2)} <= wants
    assert {dom.GEN % (1, xl, 0, 1, 0) for xl in (0, 1)} | {dom.GEN % (1, 1, 1, fa, 1) for fa in (1, 2)} <= wants
    assert {dom.GEN % (4, xl, cl, 0, 0) for xl in (0, 1) for cl in (0, 1)} <= wants


WORK = list(dom.workloads())


@pytest.mark.parametrize('w', WORK, ids=[w[0] for w in WORK])
def test_oracle_workload_runs_clean_converges_and_is_quick(orc, w):
    tag, fam, n, R, seed, first, iters, phase1, X0, converges = w
    funcs = problem(fam, n)
    prob = orc.Problem(funcs)
    if X0 is None:
        X0 = orc.keyed_normal_matrix(seed, n, R, first_index=first)

    def run(r):
        rng = orc.Rng(orc.RNG_KEYED, seed)
        rng.set_restart(first + r)
        return prob.improve_cd_sep(X0[:, r], num_iters=iters, phase1=phase1, rng=rng)       # raises on an error code
    t0 = time.time()
    res = oracle_map(run, range(R))
    dt = time.time() - t0
    print('%-28s n %5d R %2d  %.3f s' % (tag, n, R, dt))
    if converges:
        for r, (x, s1, s2) in enumerate(res):
            assert s1[0] < iters and s2[0] < iters, (tag, r, s1, s2)
    if phase1:
        assert any(s2[0] > 0 for _, _, s2 in res) or iters == 0, (tag, 'no restart reaches phase 2')
    else:           # the gate cases: some restarts pass the gate, some do not
        assert any(s2[0] > 0 for _, _, s2 in res) and any(s2[0] == 0 for _, _, s2 in res), (tag, [int(s2[0]) for _, _, s2 in res])
    assert dt < BUDGET_S, (tag, dt)


PIN = [('boxz', 32), ('boxz', 24), ('boxmix', 33), ('boxmix', 32), ('classes23', 33), ('classes23', 32), ('mixed2', 24), ('mixed3', 33),
       ('ties_bls', 32), ('ties_ann', 24), ('box', 16), ('box', 1)]


@pytest.mark.parametrize('fam,n', PIN, ids=['%s-%d' % p for p in PIN])
def test_fast_oracle_follows_the_restatement_on_the_grid_families(orc, fam, n):
    funcs = problem(fam, n)
    prob = orc.Problem(funcs)
    ties = fam.startswith('ties')
    p2 = 0
    for ci, (phase1, iters, start) in enumerate([(True, 4 if ties else 1000, 'normal')] * 3 + [(True, 0, 'normal'), (True, 1, 'normal'),
                                                (True, 2, 'normal'), (False, 4 if ties else 1000, 'gate'), (False, 2, 'gate')]):
        if start == 'normal':
            x0 = orc.keyed_normal_matrix(7, n, 1, first_index=ci)[:, 0]
        else:
            x0 = dom.gate_starts(n, 8)[:, ci]
        out = []
        for fn in (prob.improve_cd, prob.improve_cd_sep):
            rng = orc.Rng(orc.RNG_KEYED, 7)
            rng.set_restart(ci)
            out.append(fn(x0, num_iters=iters, phase1=phase1, rng=rng))
        (xa, a1, a2), (xb, b1, b2) = out
        where = (fam, n, phase1, iters, start)
        assert list(a1) == list(b1) and list(a2) == list(b2), (where, a1, b1, a2, b2)
        assert np.max(np.abs(xa - xb)) <= 1e-12 * max(1.0, np.max(np.abs(xa))), where
        if a2[0] == 0:
            assert np.array_equal(xa, xb), where
        p2 += a2[0] > 0
    assert p2 >= 3, (fam, n, p2)
