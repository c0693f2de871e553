"""The small-problem batch with PER-PROBLEM constraint coefficients (qcqpmi_cd_small_batch_run_pc, qcqpmi_sdr_small_batch_pc,
QCQPBatch.cons) without a GPU: the two symbols are declared, bound and exported and the ABI version did not move; the generator
problems.per_problem_constraints_batch is deterministic and problem b depends on seeds[b] alone; QCQPBatch builds cons for problems
that differ in their coefficients, keeps cons = None for shared constraints and refuses a differing structure; and the two
yardsticks of tests/test_gpu_small_batch_pc.py:
  * the oracle's fast separable improve_cd_sep equals the restatement improve_cd on the six families at n = 1, 2, 15, 16, 17, 33, 64
    (points bit-equal or within 1e-12, equal stats) and is not chaotic there (one ulp on x0 moves no counter and no point by 1e-9):
    what licenses the GPU comparison of EVERY restart;
  * the NumPy restatement of the mixing method (tests/sdr_batch_cases.py) certifies every eqpp problem of the GPU SDR test -- n in
    {1, 7, 32, 33, 64}, d ~ U(0.25, 4), the generator's full range, not shrunk -- ten times inside the project's threshold
    lambda_min >= -1e-6 (1 + max |C|) and under the sweep limit: the margin that file demonstrates for the shared family.
On the commit before the feature the symbols, the generator and QCQPBatch.cons are missing and these tests fail."""
import os
import re

import numpy as np
import pytest

import sdr_batch_cases as sc
import small_batch_pc_cases as pc
from conftest import REPO, oracle_map

NS = (1, 2, 15, 16, 17, 33, 64)
FAMILIES = pc.FAMILIES


def test_symbols_in_header_binding_and_library():
    with open(os.path.join(REPO, 'include', 'qcqp_mi.h')) as f:
        header = f.read()
    assert re.search(r'#define\s+QCQPMI_ABI_VERSION\s+6\b', header)
    from qcqp_amd import _ffi
    lib = _ffi.lib()
    assert lib.qcqpmi_abi_version() == 6
    for symbol, nargs, old in (('qcqpmi_cd_small_batch_run_pc', 31, 'qcqpmi_cd_small_batch_run'),
                               ('qcqpmi_sdr_small_batch_pc', 18, 'qcqpmi_sdr_small_batch')):
        assert re.search(r'\bint\s+%s\s*\(' % symbol, header)
        proto = [p for p in _ffi.PROTOTYPES if p[0] == symbol]
        assert len(proto) == 1 and len(proto[0][2]) == nargs
        base = [p for p in _ffi.PROTOTYPES if p[0] == old][0]
        assert proto[0][2][:5] == base[2][:5] and proto[0][2][5] is _ffi.c_dp and proto[0][2][6:] == base[2][5:]
        assert hasattr(lib, symbol)


def test_generator_is_deterministic_and_keyed_by_the_problem_seed():
    from qcqp_amd import problems
    assert tuple(problems.PER_PROBLEM_FAMILIES) == FAMILIES

    def same(fa, fb):
        return len(fa) == len(fb) and all(np.array_equal(np.asarray(Pa.toarray() if hasattr(Pa, 'toarray') else Pa),
                                                         np.asarray(Pb.toarray() if hasattr(Pb, 'toarray') else Pb))
                                          and np.array_equal(qa, qb) and ra == rb and oa == ob
                                          for (Pa, qa, ra, oa), (Pb, qb, rb, ob) in zip(fa, fb))
    for name in FAMILIES:
        a = problems.per_problem_constraints_batch(name, 9, [3, 4, 5])
        b = problems.per_problem_constraints_batch(name, 9, [5, 3])
        assert len(a) == 3 and same(a[0], b[1]) and same(a[2], b[0])           # problem b depends on seeds[b] only
        assert same(a[1], problems.per_problem_constraints_batch(name, 9, [4])[0])
        assert not same(a[0], a[1])
        per = 2 if name in ('linpp',) else 1
        assert len(a[0]) == 1 + (9 * per if name != 'annpp' else 5 * 2 + 4)
        c = problems.per_problem_constraints_batch(name, 10, [3])[0]
        assert c[1][2] != a[0][1][2]                                           # ... and on n
    lo_hi = problems.per_problem_constraints_batch('boxpp', 64, [1])[0][1:]
    for i, (P, q, r, rel) in enumerate(lo_hi):                                 # (x - lo)(x - hi): roots lo in [-2, 1], hi - lo in [0.05, 2]
        lo, hi = sorted(np.roots([P[i, i], q[i], r]).real)
        assert rel == '<=' and -2.0 - 1e-12 <= lo <= 1.0 and 0.05 - 1e-9 <= hi - lo <= 2.0 + 1e-9
    assert np.array_equal(problems.per_problem_constraints_batch('boxpp', 9, [4])[0][0][0], problems.box_qp(9, seed=4)[0][0][0])
    with pytest.raises(KeyError):
        problems.per_problem_constraints_batch('box', 4, [1])


def test_qcqpbatch_builds_cons_and_checks_the_structure(monkeypatch):
    import scipy.sparse as sp
    from qcqp_amd import batch, problems
    made = []
    monkeypatch.setattr(batch, 'Engine', lambda form, device=0: made.append(form) or object())     # no GPU here
    for name in FAMILIES:
        fl = problems.per_problem_constraints_batch(name, 8, [1, 2, 3])
        qb = batch.QCQPBatch(fl)
        m = len(fl[0]) - 1
        assert qb.cons.shape == (3, m, 3) and qb.cons.dtype == np.float64
        assert np.array_equal(qb.cons, pc.cons_of(fl)), name
        for k, (P, q, r, rel) in enumerate(fl[2][1:]):          # p = P_k[i,i], q = q_k[i] on the touched coordinate, r
            i = pc.entry(P, q)[0]
            assert tuple(qb.cons[2, k]) == (P[i, i], q[i], r), (name, k)
        assert not np.array_equal(qb.cons[0], qb.cons[1])
    assert len(made) == len(FAMILIES)
    shared = problems.box_qp_batch(8, [1, 2, 3], lo=0.0, hi=1.0)
    assert batch.QCQPBatch(shared).cons is None
    assert batch.QCQPBatch(problems.boolean_least_squares_batch(3, 8, 12, seed=1)).cons is None
    assert batch.QCQPBatch([problems.box_qp(8, seed=sd, lo=0.0, hi=1.0)[0] for sd in (1, 2)]).cons is None      # equal, not shared objects
    fl = problems.per_problem_constraints_batch('boxpp', 8, [1, 2, 3])
    P, q, r, rel = fl[2][3]
    for bad in ((P, q, r, '=='),                                                                   # another relop
                (sp.csr_matrix(([1.0], ([5], [5])), shape=(8, 8)), np.roll(q, 3), r, rel)):      # another coordinate
        other = fl[2][:3] + [bad] + fl[2][4:]
        with pytest.raises(Exception) as ex:
            batch.QCQPBatch([fl[0], fl[1], other])
        assert 'problem 2' in str(ex.value) and 'constraints' in str(ex.value)
    with pytest.raises(Exception) as ex:                                                           # another number of constraints
        batch.QCQPBatch([fl[0], fl[1][:-1]])
    assert 'problem 1' in str(ex.value) and 'constraints' in str(ex.value)
    Pc = np.zeros((8, 8))
    Pc[0, 1] = Pc[1, 0] = 0.5                                                                      # coupled constraints that differ
    with pytest.raises(Exception) as ex:
        batch.QCQPBatch([fl[0] + [(Pc, np.zeros(8), -1.0, '<=')], fl[1] + [(Pc, np.zeros(8), -2.0, '<=')]])
    assert 'constraints' in str(ex.value)


def test_lifted_cost_batch_broadcasts_over_d():
    from qcqp_amd import problems, sdr
    fl = problems.per_problem_constraints_batch('eqpp', 7, [1, 2, 3])
    P0s, q0s, r0s = sc.objectives(fl)
    ds = np.stack([sc.d_of(f) for f in fl])
    C = sdr.lifted_cost_batch(P0s, q0s, r0s, ds)
    for b in range(3):
        assert np.array_equal(C[b], sc.lifted(P0s[b:b + 1], q0s[b:b + 1], r0s[b:b + 1], ds[b])[0])
    assert np.array_equal(sdr.lifted_cost_batch(P0s, q0s, r0s, ds[0]), sc.lifted(P0s, q0s, r0s, ds[0]))


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
def test_fast_oracle_equals_the_restatement_on_the_families(orc, name):
    from qcqp_amd import problems

    def one(n):
        for b, funcs in enumerate(problems.per_problem_constraints_batch(name, n, [5, 6, 7])):
            for (xs, s1, s2), (xr, r1, r2) in _runs(orc, funcs, n, 4, 31 + b):
                assert np.array_equal(xs, xr) or np.max(np.abs(xs - xr) / (1 + np.abs(xr))) <= 1e-12, (name, n, b)
                assert np.array_equal(s1, r1) and np.array_equal(s2, r2), (name, n, b, s1, r1, s2, r2)
    oracle_map(one, sorted(NS, reverse=True))


@pytest.mark.parametrize('name', FAMILIES)
def test_families_are_not_chaotic(orc, name):
    """One ulp on every coordinate of x0, in either direction, oracle against oracle: the same counters and the same point to 1e-9.
    No case is left out, so the GPU test compares every restart."""
    from qcqp_amd import problems

    def one(n):
        for b, funcs in enumerate(problems.per_problem_constraints_batch(name, n, [5, 6, 7])):
            base = _runs(orc, funcs, n, 4, 77 + b)
            for bump in (np.inf, -np.inf):
                for (a, _), (c, _) in zip(base, _runs(orc, funcs, n, 4, 77 + b, bump=bump)):
                    assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2]), (name, n, b)
                    assert np.max(np.abs(a[0] - c[0]) / (1 + np.abs(c[0]))) < 1e-9, (name, n, b)
    oracle_map(one, sorted(NS, reverse=True))


def test_numpy_mixing_certifies_eqpp_with_a_tenfold_margin(orc):
    from qcqp_amd import problems

    def solve(case):
        n, B, pseeds, seed, stride, fi = case
        fl = problems.per_problem_constraints_batch('eqpp', n, pseeds)
        P0s, q0s, r0s = sc.objectives(fl)
        C = np.concatenate([sc.lifted(P0s[b:b + 1], q0s[b:b + 1], r0s[b:b + 1], sc.d_of(fl[b])) for b in range(B)])
        V, sweeps = sc.mixing_numpy(C, sc.keyed_starts(orc, B, n + 1, seed, stride))
        worst = min(sc.certificate(C[b], V[b])[1] / (1.0 + np.max(np.abs(C[b]))) for b in range(B))
        return case, worst, int(sweeps.max())
    cases = pc.sdr_cases()
    assert len(cases) == 15 and all(c[2] == big[2][:c[1]] and c[3:] == big[3:] for c in cases for big in cases if big[0] == c[0] and big[1] == 64)
    res = oracle_map(solve, sorted((c for c in cases if c[1] == 64), key=lambda c: -c[0]))      # the batches of 1 and 3 are its first problems
    assert len(res) == len(pc.SDR_NS)
    print('worst lambda_min / scale %.3e, most sweeps %d' % (min(r[1] for r in res), max(r[2] for r in res)))
    for case, worst, most in res:
        assert worst >= -1e-7, (case[:2], worst)        # ten times inside -1e-6 (1 + max |C|)
        assert most < sc.MAX_SWEEPS, (case[:2], most)
