"""The host side of improve chains (QCQPBatch.improve with a list; qcqpmi_chain_small_batch_run), without a device:
  * chain_stages, the pure function that turns improve()'s method / keyword arguments into stage descriptors: the defaults per
    method, the tuple form, the refusals;
  * the oracle's composition that tests/test_gpu_chain_batch.py holds the kernel against: a one-stage chain is the single oracle
    call, and over the cases of the GPU test it moves by less than admm_batch_cases.SENSITIVITY under a last-bit perturbation of the
    starts -- why 1e-9 is a fair threshold there (five ADMM iterations per phase: the stable horizon)."""
import numpy as np
import pytest

import admm_batch_cases as ab
import chain_batch_cases as cc
import small_batch_pc_cases as pc
from conftest import oracle_map


def test_stage_defaults_per_method():
    from qcqp_amd import settings as s
    from qcqp_amd.batch import chain_stages
    cd, admm = chain_stages([s.COORD_DESCENT, s.ADMM])
    assert cd == dict(method=s.COORD_DESCENT, phase1=True, num_iters=1000, tol=1e-4, viol_tol=1e-2, viol_lim=1e4)
    assert admm == dict(method=s.ADMM, phase1=True, num_iters=1000, tol=1e-2, viol_tol=1e-2, viol_lim=1e4)
    # a scalar is a chain of one; the call's keyword arguments are every stage's default
    assert chain_stages(s.ADMM) == [admm]
    a, b = chain_stages([s.ADMM, s.COORD_DESCENT], num_iters=7, tol=0.5, phase1=False, viol_tol=0.25, viol_lim=9.0)
    for g in (a, b):
        assert (g['num_iters'], g['tol'], g['phase1'], g['viol_tol'], g['viol_lim']) == (7, 0.5, False, 0.25, 9.0)
    assert isinstance(a['num_iters'], int) and isinstance(a['tol'], float) and isinstance(a['phase1'], bool)


def test_stage_tuple_form():
    from qcqp_amd import settings as s
    from qcqp_amd.batch import chain_stages
    # the reference's improve(COORD_DESCENT); improve(ADMM, phase1=False)
    cd, admm = chain_stages([s.COORD_DESCENT, (s.ADMM, dict(phase1=False))], num_iters=100)
    assert cd['phase1'] is True and admm['phase1'] is False and cd['num_iters'] == admm['num_iters'] == 100
    assert cd['tol'] == 1e-4 and admm['tol'] == 1e-2
    a, c = chain_stages([(s.ADMM, dict(num_iters=5, tol=1e-3, viol_lim=10.0)), (s.COORD_DESCENT, dict(viol_tol=0.5))], num_iters=100)
    assert (a['num_iters'], a['tol'], a['viol_lim']) == (5, 1e-3, 10.0) and (c['num_iters'], c['tol'], c['viol_tol']) == (100, 1e-4, 0.5)
    # a stage's own tol=None falls back to its method's default, not to the call's
    assert chain_stages([(s.ADMM, dict(tol=None))], tol=0.5)[0]['tol'] == 1e-2
    # the argument is not modified
    kw = dict(phase1=False)
    entry = [(s.ADMM, kw)]
    chain_stages(entry)
    assert kw == dict(phase1=False) and entry == [(s.ADMM, kw)]


def test_stage_refusals():
    from qcqp_amd import settings as s
    from qcqp_amd.batch import chain_stages
    with pytest.raises(Exception, match='empty'):
        chain_stages([])
    for bad in (s.DCCP, 'newton', None, (s.ADMM, 3)):
        with pytest.raises(Exception, match='defined for the COORD_DESCENT and ADMM methods'):
            chain_stages([s.ADMM, bad])
    with pytest.raises(Exception, match='defined for the COORD_DESCENT and ADMM methods'):
        chain_stages(s.DCCP)
    with pytest.raises(Exception, match="stage 1 has the argument 'rho'"):
        chain_stages([s.ADMM, (s.ADMM, dict(rho=1.0))])


def test_cases_cover_what_the_kernel_distinguishes():
    assert set(cc.NS) == {1, 2, 33, 63, 64}
    assert [k[3] for k in cc.KINDS] == ['<1>', '<4>', '<1,pc>', '<4,pc>']
    assert [len(v) for _, v in sorted(cc.CHAINS.items())] == [2, 4, 2, 2]
    assert all(g['num_iters'] == 100 for v in cc.CHAINS.values() for g in v)
    for kind in cc.KINDS:      # every kind exists at the smallest and at the largest size, with the coefficients the label promises
        for n in (1, 64):
            fl, cons = cc.problems_of(kind, n, 2, seed=3)
            assert len(fl) == 2 and (cons is not None) == kind[1]
            per_coord = np.bincount([pc.entry(P, q)[0] for P, q, _, _ in fl[0][1:]], minlength=n)
            assert per_coord.max() == (2 if kind[0].startswith('two') else 1), (kind, n, per_coord)


def test_oracle_chain_of_one_stage_is_the_single_call(orc):
    fl = ab.family('bls', 17, 2, seed=4)
    X0 = ab.starts(orc, 9, 3, 2, 2, 3, 17)
    _, _, _, rhos, _ = cc.host_side(fl)
    for b in range(2):
        prob = orc.Problem(fl[b])
        for r in range(3):
            sd = ab.seed_of(9, 3, b)
            (rec,) = cc.oracle_chain(orc, prob, X0[b, r], sd, 2 + r, [cc.stage(cc.ADMM, num_iters=ab.NUM_ITERS)], float(rhos[b]))
            x, i1, i2 = ab.improve_admm(prob, X0[b, r], num_iters=ab.NUM_ITERS, rho=float(rhos[b]))
            assert np.array_equal(rec['x'], x) and (rec['iters1'], rec['iters2']) == (i1, i2)
            (rec,) = cc.oracle_chain(orc, prob, X0[b, r], sd, 2 + r, [cc.stage(cc.CD)], float(rhos[b]))
            rng = orc.Rng(orc.RNG_KEYED, sd)
            rng.set_restart(2 + r)
            x, s1, s2 = prob.improve_cd_sep(X0[b, r], num_iters=cc.NUM_ITERS, rng=rng)
            assert np.array_equal(rec['x'], x) and np.array_equal(rec['s1'], s1) and np.array_equal(rec['s2'], s2)
            assert rec['f0'] == prob.eval(0, x) and rec['maxviol'] == prob.max_violation(x)


@pytest.mark.parametrize('c', [c for c in cc.oracle_cases() if c[2] < 64], ids=cc.oracle_case_id)
def test_oracle_chain_is_stable_on_the_cases_of_the_gpu_test(orc, c):
    """A last-bit perturbation of the starts moves no stage of the oracle's chain by more than SENSITIVITY and changes no count.
    (n = 2 and 33 of the GPU test's sizes: this file is collected ahead of tests/test_host_cpu.py, whose rendezvous test wants a
    young session, so it stays under a second; n = 64 moves by 8e-15 at the most.)"""
    label, name, n, ps, seed, stride, fi = c
    stages = cc.ORACLE_CHAINS[label]
    fl = ab.family(name, n, cc.ORACLE_B, seed=ps)
    _, _, _, rhos, _ = cc.host_side(fl)
    X0 = ab.starts(orc, seed, stride, fi, cc.ORACLE_B, cc.ORACLE_R, n)
    a = cc.oracle_chain_batch(orc, oracle_map, fl, X0, stages, rhos, seed, stride, fi)
    p = cc.oracle_chain_batch(orc, oracle_map, fl, ab.perturbed(X0), stages, rhos, seed, stride, fi)
    worst = 0.0
    for b in range(cc.ORACLE_B):
        for r in range(cc.ORACLE_R):
            for g, ra, rp in zip(stages, a[b][r], p[b][r]):
                worst = max(worst, ab.rel(rp['x'], ra['x']))
                for key in ('iters1', 'iters2') if g['method'] == cc.ADMM else ('s1', 's2'):
                    assert np.array_equal(ra[key], rp[key]), (c, b, r, key)
    print('\n%s: the oracle moves by %.1e' % (cc.oracle_case_id(c), worst))
    assert worst < ab.SENSITIVITY, (c, worst)
