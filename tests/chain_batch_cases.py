"""What tests/test_chain_batch_cpu.py and tests/test_gpu_chain_batch.py share: the chains, the grid of qcqpmi_chain_small_batch_run's
domain, the COMPOSED yardstick (the single engine calls stage by stage, X of one as X0 of the next) and the oracle's composition
(improve_admm / improve_cd_sep one after the other from the same keyed start with the same keyed rng).  A plain module, not a conftest."""
import numpy as np

import admm_batch_cases as ab

CD, ADMM = 0, 1                              # qcqpmi_chain_stage.method
NS = (1, 2, 33, 63, 64)
NUM_ITERS = 100                              # the bit-for-bit tests run at full length
CD_KEYS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')
ADMM_KEYS = ('iters1', 'iters2')
FINAL_KEYS = ('f0', 'maxviol', 'X', 'best_index', 'best_f0', 'best_maxviol', 'best_x')
# constraint lists: (label, per-problem coefficients?, family, the kernel's template arguments as qcqpmi_last_cd_kernel names them)
KINDS = (('one', False, 'bls', '<1>'), ('two', False, 'ann2', '<4>'), ('one-pc', True, 'boxpp', '<1,pc>'), ('two-pc', True, 'annpp', '<4,pc>'))


def stage(method, num_iters=NUM_ITERS, phase1=True, tol=None, viol_tol=1e-2, viol_lim=1e4):
    """One stage as Engine.chain_small_batch_run takes it; tol == None: the method's own default."""
    return dict(method=method, phase1=phase1, num_iters=num_iters, tol=(1e-4 if method == CD else 1e-2) if tol is None else tol,
                viol_tol=viol_tol, viol_lim=viol_lim)


CHAINS = {
    'admm-cd': [stage(ADMM), stage(CD)],
    'cd-admm2': [stage(CD), stage(ADMM, phase1=False)],
    'cd-cd': [stage(CD), stage(CD)],
    'admm-cd-admm-cd': [stage(ADMM), stage(CD), stage(ADMM), stage(CD)],
}
# against the oracle ADMM runs five iterations per phase: the stable horizon of admm_batch_cases
ORACLE_CHAINS = {
    'admm5-cd': [stage(ADMM, num_iters=ab.NUM_ITERS), stage(CD)],
    'cd-admm5': [stage(CD), stage(ADMM, num_iters=ab.NUM_ITERS, phase1=False)],
}
ORACLE_NS = (2, 33, 64)
ORACLE_FAMILIES = ('bls', 'box')             # x_i^2 == 1 and (x_i + 1)(x_i - 1) <= 0
ORACLE_B, ORACLE_R = 3, 4


def problems_of(kind, n, B, seed=1):
    """(funcs list, cons or None) of a constraint kind of KINDS."""
    _, pc, name, _ = kind
    if pc:
        fl = ab.pc_family(name, n, B, seed=seed)
        return fl, ab.cons_of(fl)
    return ab.family(name, n, B, seed=seed), None


def host_side(fl, rho=None):
    """P0s, q0s, r0s, rhos, Minvs as QCQPBatch computes them on the host."""
    from qcqp_amd import batch
    P0s, q0s, r0s = ab.objectives(fl)
    m = len(fl[0]) - 1
    rhos = batch.admm_rhos(P0s, m, rho)
    return P0s, q0s, r0s, rhos, batch.admm_minvs(P0s, rhos, m)


def composed(e, host, R, stages, X0=None, seed=0, stride=1, fi=0, cons=None):
    """The yardstick: Engine.cd_small_batch_run / admm_small_batch_run stage by stage.  The dictionary of the last call, with 'stages'
    (per stage its records, f0, maxviol) and 'X' of the last stage."""
    P0s, q0s, r0s, rhos, Minvs = host
    X, per_stage, out = X0, [], None
    for g in stages:
        kw = dict(X0=X, phase1=g['phase1'], num_iters=g['num_iters'], tol=g['tol'], seed=seed, seed_stride=stride, first_index=fi, cons=cons)
        if g['method'] == ADMM:
            out = e.admm_small_batch_run(P0s, q0s, r0s, R, rhos, Minvs, viol_lim=g['viol_lim'], **kw)
            keys = ADMM_KEYS
        else:
            out = e.cd_small_batch_run(P0s, q0s, r0s, R, viol_tol=g['viol_tol'], **kw)
            keys = CD_KEYS
        X = out['X']
        per_stage.append(dict((k, out[k]) for k in keys + ('f0', 'maxviol')))
    out = dict(out)
    out['stages'] = per_stage
    return out


def fused(e, host, R, stages, X0=None, seed=0, stride=1, fi=0, cons=None):
    P0s, q0s, r0s, rhos, Minvs = host
    return e.chain_small_batch_run(P0s, q0s, r0s, R, stages, rhos=rhos, Minvs=Minvs, X0=X0, seed=seed, seed_stride=stride, first_index=fi,
                                   cons=cons)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(f, c, stages, tag):
    """Every per-stage record, the final point, objective, violation and the winners of two runs, bit for bit."""
    assert len(f['stages']) == len(c['stages']) == len(stages), tag
    for k, (fs, cs, g) in enumerate(zip(f['stages'], c['stages'], stages)):
        for key in (ADMM_KEYS if g['method'] == ADMM else CD_KEYS) + ('f0', 'maxviol'):
            assert same_bits(fs[key], cs[key]), (tag, 'stage', k, key, int(np.count_nonzero(np.asarray(fs[key]) != np.asarray(cs[key]))))
    for key in (ADMM_KEYS if stages[-1]['method'] == ADMM else CD_KEYS) + FINAL_KEYS:
        assert same_bits(f[key], c[key]), (tag, 'final', key)


def given_starts(B, R, n, seed):
    """X0 (B, R, n) that is not the keyed normals."""
    return np.random.RandomState(seed).uniform(-2.0, 2.0, size=(B, R, n))


# ---- the oracle's composition

def oracle_chain(orc, prob, x0, sd, gidx, stages, rho):
    """The stages one after the other on one restart: improve_admm (admm_batch_cases) or improve_cd_sep with the keyed rng
    (sd, gidx) -- every CD stage a fresh one, as two calls with the same seed draw.  Per stage a dictionary: x, f0, maxviol and
    iters1 / iters2 or the oracle's s1 / s2."""
    x, out = np.ascontiguousarray(x0, dtype=np.float64), []
    for g in stages:
        if g['method'] == ADMM:
            x, i1, i2 = ab.improve_admm(prob, x, num_iters=g['num_iters'], viol_lim=g['viol_lim'], tol=g['tol'], rho=rho, phase1=g['phase1'])
            rec = dict(iters1=i1, iters2=i2)
        else:
            rng = orc.Rng(orc.RNG_KEYED, sd)
            rng.set_restart(gidx)
            x, s1, s2 = prob.improve_cd_sep(x, num_iters=g['num_iters'], viol_tol=g['viol_tol'], tol=g['tol'], phase1=g['phase1'], rng=rng)
            rec = dict(s1=s1, s2=s2)
        rec.update(x=np.array(x), f0=prob.eval(0, x), maxviol=prob.max_violation(x))
        out.append(rec)
    return out


def oracle_chain_batch(orc, oracle_map, fl, X0, stages, rhos, seed, stride, fi):
    """oracle_chain of every (problem, restart): a (B, R) nested list of the per-stage dictionaries."""
    B, R, _ = X0.shape
    probs = [orc.Problem(f) for f in fl]
    for p in probs:
        p.eig()                  # once per problem, before the threads share it

    def one(br):
        b, r = divmod(br, R)
        return oracle_chain(orc, probs[b], X0[b, r], ab.seed_of(seed, stride, b), fi + r, stages, float(rhos[b]))
    res = oracle_map(one, range(B * R))
    return [[res[b * R + r] for r in range(R)] for b in range(B)]


def oracle_cases():
    """(chain label, family, n, problem seed, seed, seed_stride, first_index)"""
    out = []
    for k0, label in enumerate(sorted(ORACLE_CHAINS)):
        for k1, name in enumerate(ORACLE_FAMILIES):
            for j, n in enumerate(ORACLE_NS):
                out.append((label, name, n, 60 + 10 * k1 + j, 17 + j + 100 * k0, 3, 5 * j))
    return out


def oracle_case_id(c):
    return '%s-%s-n%d' % c[:3]
