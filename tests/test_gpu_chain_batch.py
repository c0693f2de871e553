"""qcqpmi_chain_small_batch_run / QCQPBatch.improve([method, ...]): a chain of improve methods (COORD_DESCENT, ADMM) for B small
problems, R restarts each, in ONE launch of chain_small_kernel (csrc/chain_small.hip).

The call is DEFINED as the composition of the single calls, so the yardstick is the composed path (chain_batch_cases.composed: the
engine calls of the single methods stage by stage, X of one as X0 of the next) and the comparison is BIT FOR BIT -- the same device
functions in the same order, the library built with -ffp-contract=off: a differing bit is a finding about the hand-over between the
stages or about the move of the restart bodies into headers, never a tolerance.  Against the oracle the chain inherits the horizon of
batched ADMM (five iterations per phase, 1e-9; tests/test_chain_batch_cpu.py shows the oracle's own composition stable to 1e-11 on
these cases).  Without the feature every test here fails: the symbol does not exist and improve() refuses a list."""
import numpy as np
import pytest

import admm_batch_cases as ab
import chain_batch_cases as cc
from conftest import oracle_map
from life_oracle import make, rel

pytestmark = pytest.mark.gpu

B0, R0 = 3, 9                                # B below the workgroup count: a problem is split into several tickets


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def both(e, host, R, stages, tag, kernel=None, **kw):
    """The fused launch and the composed yardstick on one context, compared bit for bit; returns the fused dictionary."""
    f = cc.fused(e, host, R, stages, **kw)
    if kernel is not None:
        assert e.last_cd_kernel() == 'chain_small_kernel' + kernel, (tag, e.last_cd_kernel())
    c = cc.composed(e, host, R, stages, **kw)
    cc.assert_same(f, c, stages, tag)
    return f


# ---- Test 1: fused equals composed, bit for bit

@pytest.mark.parametrize('n', cc.NS)
@pytest.mark.parametrize('kind', cc.KINDS, ids=lambda k: k[0])
def test_fused_equals_composed(eng_mod, kind, n):
    fl, cons = cc.problems_of(kind, n, B0, seed=3 + n)
    host = cc.host_side(fl)
    e = make(eng_mod, fl[0])
    ran = np.zeros(2, dtype=np.int64)
    for label, stages in sorted(cc.CHAINS.items()):
        for X0 in (None, cc.given_starts(B0, R0, n, seed=n)):
            f = both(e, host, R0, stages, (kind[0], n, label, X0 is not None), kernel=kind[3], X0=X0, seed=11 + n, stride=3, fi=2, cons=cons)
            for g, st in zip(stages, f['stages']):      # the stages did run: the comparison is not one of zeros
                ran[g['method']] += int(np.sum(st['iters2'] if g['method'] == cc.ADMM else st['sweeps1'] + st['sweeps2']))
    e.close()
    assert ran[cc.CD] > 0 and ran[cc.ADMM] > 0, ran


@pytest.mark.parametrize('kind', [cc.KINDS[0], cc.KINDS[3]], ids=lambda k: k[0])
def test_one_ticket_per_problem(eng_mod, kind):
    """B = 600, R = 2 at n = 4: more problems than resident workgroups, a ticket is a whole problem."""
    B, R, n = 600, 2, 4
    fl, cons = cc.problems_of(kind, n, B, seed=7)
    host = cc.host_side(fl)
    e = make(eng_mod, fl[0])
    for label in ('admm-cd', 'admm-cd-admm-cd'):
        both(e, host, R, cc.CHAINS[label], (kind[0], 'B600', label), kernel=kind[3], seed=5, stride=1, cons=cons)
    e.close()


def test_a_failed_restart_hands_its_point_on(eng_mod):
    """A coordinate without a constraint under phase 1 of coordinate descent: the reference raises, the stage reports status1 = -3 and
    f0 = maxviol = inf for every restart -- and the next stage still starts from the point the failed stage wrote."""
    n, B, R = 16, 3, 5
    fl = [f[:-1] for f in ab.family('bls', n, B, seed=2)]
    host = cc.host_side(fl)
    e = make(eng_mod, fl[0])
    for stages in ([cc.stage(cc.CD), cc.stage(cc.ADMM, phase1=False)], [cc.stage(cc.CD), cc.stage(cc.ADMM)]):
        f = both(e, host, R, stages, ('failed', len(stages)), kernel='<1>', seed=2)
        first = f['stages'][0]
        assert (first['status1'] == -3).all() and (first['ran_phase2'] == 0).all() and np.isinf(first['f0']).all() and np.isinf(first['maxviol']).all()
        assert np.isfinite(f['stages'][1]['f0']).all() and (f['stages'][1]['iters2'] >= 1).all()
        # the point handed on is the one the failed stage left: the second stage alone, from the first stage's X
        P0s, q0s, r0s, rhos, Minvs = host
        x1 = e.cd_small_batch_run(P0s, q0s, r0s, R, seed=2, num_iters=cc.NUM_ITERS)['X']
        g = stages[1]
        o2 = e.admm_small_batch_run(P0s, q0s, r0s, R, rhos, Minvs, X0=x1, phase1=g['phase1'], num_iters=g['num_iters'], seed=2)
        assert cc.same_bits(o2['f0'], f['stages'][1]['f0']) and cc.same_bits(o2['iters2'], f['stages'][1]['iters2'])
    e.close()


@pytest.mark.parametrize('ex', [x for x in ab.exit_cases() if x[0] in ('phase2-by-viol-lim', 'phase2-by-tol', 'one-iteration')], ids=lambda x: x[0])
def test_an_admm_stage_that_leaves_early_hands_its_point_on(eng_mod, orc, ex):
    """The starts and arguments of admm_batch_cases.exit_cases drive the ADMM stage out of its loop at once; coordinate descent goes on."""
    label, name, n, ps, kw, want = ex
    fl = ab.family(name, n, 2, seed=ps)
    host = cc.host_side(fl)
    stages = [cc.stage(cc.ADMM, **kw), cc.stage(cc.CD)]
    e = make(eng_mod, fl[0])
    f = both(e, host, ab.EXIT_R, stages, label, seed=31, stride=3)
    e.close()
    assert want(f['stages'][0]['iters1'], f['stages'][0]['iters2']), (f['stages'][0]['iters1'], f['stages'][0]['iters2'])


# ---- Test 2: invariances, bit for bit

@pytest.mark.parametrize('kind', [cc.KINDS[0], cc.KINDS[3]], ids=lambda k: k[0])
def test_invariance_bit_for_bit(eng_mod, kind):
    B, R, n = 7, 8, 33
    stages = cc.CHAINS['admm-cd-admm-cd']
    fl, cons = cc.problems_of(kind, n, B, seed=21)
    host = cc.host_side(fl)
    e = make(eng_mod, fl[0])

    def sub(idx):
        return tuple(a[idx] for a in host), (None if cons is None else cons[idx])

    def check(a, ia, b, ib, tag):
        for k, (sa, sb, g) in enumerate(zip(a['stages'], b['stages'], stages)):
            for key in (cc.ADMM_KEYS if g['method'] == cc.ADMM else cc.CD_KEYS) + ('f0', 'maxviol'):
                assert cc.same_bits(sa[key][ia], sb[key][ib]), (tag, k, key)
        for key in cc.FINAL_KEYS:
            assert cc.same_bits(a[key][ia], b[key][ib]), (tag, key)

    o = cc.fused(e, host, R, stages, seed=4, stride=2, fi=1, cons=cons)
    for b in (0, 3, B - 1):                   # the batch of one
        h1, c1 = sub(slice(b, b + 1))
        o1 = cc.fused(e, h1, R, stages, seed=4 + 2 * b, stride=2, fi=1, cons=c1)
        check(o, b, o1, 0, ('one', b))
    perm = np.arange(B)[::-1].copy()          # the problems in reversed order (one seed for all: stride 0)
    oa = cc.fused(e, host, R, stages, seed=4, stride=0, fi=1, cons=cons)
    hp, cp = sub(perm)
    ob = cc.fused(e, hp, R, stages, seed=4, stride=0, fi=1, cons=cp)
    check(oa, perm, ob, slice(None), 'reversed')
    h0 = cc.fused(e, host, R // 2, stages, seed=4, stride=2, fi=1, cons=cons)      # R at first_index 1 = R / 2 at 1 and at 1 + R / 2
    h1 = cc.fused(e, host, R // 2, stages, seed=4, stride=2, fi=1 + R // 2, cons=cons)
    for k, g in enumerate(stages):
        for key in (cc.ADMM_KEYS if g['method'] == cc.ADMM else cc.CD_KEYS) + ('f0', 'maxviol'):
            assert cc.same_bits(o['stages'][k][key], np.concatenate([h0['stages'][k][key], h1['stages'][k][key]], axis=1)), ('split', k, key)
    for key in ('f0', 'maxviol', 'X'):
        assert cc.same_bits(o[key], np.concatenate([h0[key], h1[key]], axis=1)), ('split', key)
    e.close()


# ---- Test 3: the oracle

@pytest.mark.parametrize('c', cc.oracle_cases(), ids=cc.oracle_case_id)
def test_against_the_oracle(eng_mod, orc, c):
    """improve_admm then improve_cd_sep (or the reverse) of the oracle from the same keyed start with the same keyed rng: points,
    counts, objective and violation of every stage of every restart to 1e-9 (admm_batch_cases.PARITY)."""
    label, name, n, ps, seed, stride, fi = c
    stages = cc.ORACLE_CHAINS[label]
    B, R = cc.ORACLE_B, cc.ORACLE_R
    fl = ab.family(name, n, B, seed=ps)
    host = cc.host_side(fl)
    e = make(eng_mod, fl[0])
    f = both(e, host, R, stages, cc.oracle_case_id(c), seed=seed, stride=stride, fi=fi)
    # every stage's points: the composed path with the same bits hands them out
    Xs = []
    X = None
    P0s, q0s, r0s, rhos, Minvs = host
    for g in stages:
        kw = dict(X0=X, phase1=g['phase1'], num_iters=g['num_iters'], tol=g['tol'], seed=seed, seed_stride=stride, first_index=fi)
        X = (e.admm_small_batch_run(P0s, q0s, r0s, R, rhos, Minvs, viol_lim=g['viol_lim'], **kw) if g['method'] == cc.ADMM
             else e.cd_small_batch_run(P0s, q0s, r0s, R, viol_tol=g['viol_tol'], **kw))['X']
        Xs.append(X)
    e.close()
    assert cc.same_bits(Xs[-1], f['X'])
    want = cc.oracle_chain_batch(orc, oracle_map, fl, ab.starts(orc, seed, stride, fi, B, R, n), stages, rhos, seed, stride, fi)
    worst = dict(x=0.0, f0=0.0, maxviol=0.0)
    for b in range(B):
        for r in range(R):
            for k, (g, st, w) in enumerate(zip(stages, f['stages'], want[b][r])):
                tag = (cc.oracle_case_id(c), b, r, k)
                worst['x'] = max(worst['x'], rel(Xs[k][b, r], w['x']))
                worst['f0'] = max(worst['f0'], abs(st['f0'][b, r] - w['f0']) / (1.0 + abs(w['f0'])))
                worst['maxviol'] = max(worst['maxviol'], abs(st['maxviol'][b, r] - w['maxviol']))
                if g['method'] == cc.ADMM:
                    assert (st['iters1'][b, r], st['iters2'][b, r]) == (w['iters1'], w['iters2']), tag
                else:
                    s1, s2 = w['s1'], w['s2']
                    assert st['sweeps1'][b, r] == s1[0] or (s1[0] == g['num_iters'] and not st['ran_phase2'][b, r]), tag
                    assert bool(st['ran_phase2'][b, r]) == (s2[0] > 0), tag
                    assert st['visits2'][b, r] == s2[1] and st['accepted2'][b, r] == s2[2], tag
                    assert st['status1'][b, r] == 0 and st['status2'][b, r] == 0, tag
    print('\n%s: against the oracle point %.1e, f0 %.1e, max violation %.1e' % (cc.oracle_case_id(c), worst['x'], worst['f0'], worst['maxviol']))
    assert max(worst.values()) < ab.PARITY, (c, worst)


# ---- Test 4: the facade

def engine_composition(eng_mod, fl, R, stages, seed, stride, fi, X0=None):
    host = cc.host_side(fl)
    e = make(eng_mod, fl[0])
    o = cc.composed(e, host, R, stages, X0=X0, seed=seed, stride=stride, fi=fi)
    e.close()
    return o, host[3]


def test_facade_list_equals_the_composition_of_engine_calls(eng_mod):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 5, 64, 6, 17
    fl = ab.family('bls', n, B, seed=2)
    o, rhos = engine_composition(eng_mod, fl, R, [cc.stage(cc.ADMM), cc.stage(cc.CD)], seed, 2, 3)
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3, seed_stride=2)
    seen = {}
    for fused in (None, False):
        f, v = qb.improve([s.ADMM, s.COORD_DESCENT], num_iters=cc.NUM_ITERS, fused=fused)
        st = qb.last_stats
        assert st['fused'] is (fused is None) and st['method'] == [s.ADMM, s.COORD_DESCENT] and st['num_restarts'] == R
        assert st['kernel'] == ('chain_small_kernel<1>' if fused is None else 'admm_small_kernel<1> + cd_small_kernel<1>'), st['kernel']
        assert cc.same_bits(f, o['best_f0']) and cc.same_bits(v, o['best_maxviol']) and cc.same_bits(qb.x, o['best_x'])
        assert cc.same_bits(qb.best_index, o['best_index']) and cc.same_bits(qb.population_f, o['f0']) and cc.same_bits(qb.population_v, o['maxviol'])
        assert cc.same_bits(st['rho'], rhos) and st['setup'] == 'host'
        assert [g['method'] for g in st['stages']] == [s.ADMM, s.COORD_DESCENT]
        for key in cc.ADMM_KEYS + ('f0', 'maxviol'):
            assert cc.same_bits(st['stages'][0][key], o['stages'][0][key]), key
        for key in cc.CD_KEYS + ('f0', 'maxviol'):
            assert cc.same_bits(st['stages'][1][key], o['stages'][1][key]) and cc.same_bits(st[key], o[key]), key
        assert st['failed_restarts'] == 0
        seen[fused] = dict((k, st[k]) for k in cc.CD_KEYS + ('f0', 'maxviol', 'best_index', 'best_f0', 'best_maxviol', 'best_x'))
    for k in seen[None]:                      # fused=False equals fused=None bit for bit at n = 64
        assert cc.same_bits(seen[None][k], seen[False][k]), k
    # the tuple form: the reference's improve(COORD_DESCENT); improve(ADMM, phase1=False)
    o2, _ = engine_composition(eng_mod, fl, R, [cc.stage(cc.CD), cc.stage(cc.ADMM, phase1=False)], seed, 2, 3)
    f, v = qb.improve([s.COORD_DESCENT, (s.ADMM, dict(phase1=False))], num_iters=cc.NUM_ITERS)
    assert qb.last_stats['fused'] is True and cc.same_bits(f, o2['best_f0']) and cc.same_bits(qb.x, o2['best_x'])
    assert cc.same_bits(qb.last_stats['iters2'], o2['iters2']) and 'failed_restarts' not in qb.last_stats
    # two separate improve() calls still each start from suggest()'s points
    f1, _ = qb.improve(s.COORD_DESCENT, num_iters=cc.NUM_ITERS)
    f2, _ = qb.improve(s.COORD_DESCENT, num_iters=cc.NUM_ITERS)
    assert cc.same_bits(f1, f2)
    qb.close()


def test_facade_scalar_calls_are_what_they_were(eng_mod):
    """improve(ADMM) and improve(COORD_DESCENT), scalar or as a list of one: the last_stats keys and values of the Engine calls."""
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 4, 33, 5, 9
    fl = ab.family('bls', n, B, seed=6)
    P0s, q0s, r0s, rhos, Minvs = cc.host_side(fl)
    e = make(eng_mod, fl[0])
    oa = e.admm_small_batch_run(P0s, q0s, r0s, R, rhos, Minvs, num_iters=30, seed=seed, want_x=False)
    oc = e.cd_small_batch_run(P0s, q0s, r0s, R, num_iters=30, seed=seed, want_x=False)
    e.close()
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=R, seed=seed)
    for method in (s.ADMM, [s.ADMM], [(s.ADMM, dict(num_iters=30))]):
        qb.improve(method, num_iters=30)
        st = qb.last_stats
        assert set(st) == set(oa) | {'method', 'num_problems', 'num_restarts', 'rho', 'kernel', 'setup', 'lambda_min', 'setup_sweeps'}, sorted(st)
        assert st['method'] == s.ADMM and st['kernel'] == 'admm_small_kernel<1>' and st['setup'] == 'host' and st['X'] is None
        assert (st['num_problems'], st['num_restarts'], st['lambda_min'], st['setup_sweeps']) == (B, R, None, None)
        for k in oa:
            assert st[k] is None if oa[k] is None else cc.same_bits(st[k], oa[k]), k
        assert cc.same_bits(st['rho'], rhos)
    for method in (s.COORD_DESCENT, [s.COORD_DESCENT]):
        qb.improve(method, num_iters=30)
        st = qb.last_stats
        assert set(st) == set(oc) | {'method', 'num_problems', 'num_restarts', 'failed_restarts', 'kernel'}, sorted(st)
        assert st['method'] == s.COORD_DESCENT and st['kernel'] == 'cd_small_kernel<1>' and st['failed_restarts'] == 0
        for k in oc:
            assert st[k] is None if oc[k] is None else cc.same_bits(st[k], oc[k]), k
    qb.close()


def test_facade_past_the_fused_kernel(eng_mod):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    # n = 65: the list runs composed on the wide kernels
    B, n, R = 2, 65, 3
    fl = ab.family('bls', n, B, seed=4)
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=R, seed=5)
    with pytest.raises(Exception, match='fused=True'):
        qb.improve([s.ADMM, s.COORD_DESCENT], wide=True, fused=True)
    with pytest.raises(Exception, match='wide=True'):
        qb.improve([s.ADMM, s.COORD_DESCENT])
    assert qb.x is None and qb.last_stats is None             # before any launch
    f, v = qb.improve([s.ADMM, s.COORD_DESCENT], num_iters=20, wide=True)
    st = qb.last_stats
    assert st['fused'] is False and st['kernel'] == 'admm_small_kernel<1,w2> + cd_small_kernel<1,w2>', st['kernel']
    P0s, q0s, r0s, rhos, Minvs = cc.host_side(fl)
    e = make(eng_mod, fl[0])
    o1 = e.admm_batch_run(P0s, q0s, r0s, R, rhos, Minvs, num_iters=20, seed=5)
    o2 = e.cd_batch_run(P0s, q0s, r0s, R, X0=o1['X'], num_iters=20, seed=5)
    e.close()
    assert cc.same_bits(f, o2['best_f0']) and cc.same_bits(qb.x, o2['best_x']) and cc.same_bits(st['stages'][0]['iters2'], o1['iters2'])
    qb.close()
    # five stages: composed with fused=None, refused with fused=True
    fl = ab.family('bls', 16, 3, seed=4)
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=4, seed=5)
    five = [s.ADMM, s.COORD_DESCENT, s.ADMM, s.COORD_DESCENT, (s.ADMM, dict(phase1=False))]
    with pytest.raises(Exception, match='at most 4 stages'):
        qb.improve(five, num_iters=20, fused=True)
    assert qb.last_stats is None
    qb.improve(five, num_iters=20)
    assert qb.last_stats['fused'] is False and len(qb.last_stats['stages']) == 5
    four = qb.improve(five[:4], num_iters=20)                 # the first four fused, then the fifth by hand: the same bits
    assert qb.last_stats['fused'] is True
    with pytest.raises(Exception, match='defined for the COORD_DESCENT and ADMM methods'):
        qb.improve([s.ADMM, s.DCCP])
    with pytest.raises(Exception, match='empty'):
        qb.improve([])
    assert four is not None
    qb.close()


# ---- Test 5: ABI refusals

def test_refusals_leave_the_population_alone(eng_mod):
    from qcqp_amd import problems

    def refused(funcs, code, stages, minvs=True):
        e = make(eng_mod, funcs)
        e.randn(19, seed=3)
        if e.n <= 64:
            e.cd_run(num_iters=2, seed=3)
        before, kern = e.download(), e.last_cd_kernel()
        B, R, n = 2, 4, e.n
        with pytest.raises(eng_mod.EngineError) as ex:
            e.chain_small_batch_run(np.zeros((B, n, n)), np.zeros((B, n)), np.zeros(B), R, stages, rhos=np.ones(B) if minvs else None,
                                    Minvs=np.stack([np.eye(n)] * B) if minvs else None)
        assert ex.value.code == code, (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before) and e.last_cd_kernel() == kern
        e.close()

    funcs = problems.boolean_least_squares(16, 20, seed=1)[0]
    two = [cc.stage(cc.ADMM, num_iters=3), cc.stage(cc.CD, num_iters=3)]
    refused(funcs, -1, [])                                                        # nstages = 0
    refused(funcs, -1, two + two + two[:1])                                       # nstages = 5
    refused(funcs, -1, two, minvs=False)                                          # an ADMM stage without rhos / Minvs
    refused(funcs, -1, [dict(two[0], method=2), two[1]])                          # an unknown method
    refused(funcs, -1, [two[0], dict(two[1], tol=0.0)])                           # what the CD call refuses
    refused(problems.boolean_least_squares(65, 70, seed=1)[0], -4, two)           # n = 65
    # a chain of CD stages needs neither rhos nor Minvs
    e = make(eng_mod, funcs)
    o = e.chain_small_batch_run(np.stack([np.eye(16)] * 2), np.zeros((2, 16)), np.zeros(2), 4, [two[1], two[1]])
    assert o['f0'].shape == (2, 4) and e.last_cd_kernel() == 'chain_small_kernel<1>'
    e.close()
