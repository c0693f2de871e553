"""The reference and the bounds of tests/eval_reference.py, checked without a GPU: the longdouble tier against exact rational
arithmetic, the float64 tier and a blocked, reversed fp64 re-ordering against their bounds, the checker against host-made WRONG
evaluations of a case from each table (every one must be refused), and the restatement of dense_zsplit on the seven shapes whose
natural K-split is 1..7."""
import numpy as np
import pytest

import eval_reference as er

# (n, m + 1, R) of the trial the bound was derived for
TRIAL_SHAPES = [(80, 64, 4096), (257, 9, 208), (130, 3, 200)]


@pytest.fixture(scope='module')
def trial():
    out = {}
    for n, m1, R in TRIAL_SHAPES:
        funcs = er.coupled_problem(n, m1 - 1, seed=n)
        X = er.population(n, R, seed=n + 1)
        out[(n, m1, R)] = (funcs, X, er.Reference(funcs, X, er.K_dense(n), seed=n))
    return out


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).nmant >= 63 or not er.LD_OK      # else the sample tier is fractions.Fraction on >= 4 columns
    assert er.U == 2.0 ** -53


def test_sample_columns_hold_the_edges():
    for R in (1, 15, 33, 200, 208, 4096):
        cols = er.sample_columns(R, seed=R)
        assert cols.size == min(R, max(32, cols.size)) and cols.size >= min(R, 32)
        assert np.all(np.diff(cols) > 0) and cols[0] == 0 and cols[-1] == R - 1
        want = {c for c in (0, 15, 16, R - 1) if 0 <= c < R}
        for j in range(1, R // 128 + 2):
            want.update(c for c in (128 * j - 1, 128 * j) if c < R)
        assert want <= set(cols.tolist()), R
        assert np.array_equal(cols, er.sample_columns(R, seed=R))      # seeded


@pytest.mark.parametrize('shape', TRIAL_SHAPES)
def test_longdouble_tier_against_exact_rational_arithmetic(trial, shape):
    funcs, X, ref = trial[shape]
    rs = np.random.RandomState(shape[0])
    entries = [(0, 0), (len(funcs) - 1, ref.cols.size - 1)] + [(int(rs.randint(len(funcs))), int(rs.randint(ref.cols.size))) for _ in range(2)]
    for k, ci in entries:
        P, q, r, rel = ref.funcs[k]
        exact = er.quad_fraction(P, q, r, X[:, ref.cols[ci]])
        # a longdouble is a dyadic rational: split it into two doubles to hand it to Fraction exactly
        hi = float(ref.FLD[k, ci])
        lo = float(ref.FLD[k, ci] - np.longdouble(hi))
        err = abs(float(er.fractions.Fraction(hi) + er.fractions.Fraction(lo) - exact))
        bound = float(ref.bound[k, ref.cols[ci]])
        assert err <= 1e-3 * bound, (shape, k, ci, err, bound)


@pytest.mark.parametrize('shape', TRIAL_SHAPES)
def test_float64_tier_and_a_reversed_blocked_order_stay_inside_the_bound(trial, shape):
    funcs, X, ref = trial[shape]
    n, m1, R = shape
    # the float64 tier is itself an fp64 evaluation of the stated shape: inside K u A of the longdouble tier
    r64 = er.worst_ratio(ref.F64[:, ref.cols], ref.FLD, ref.bound[:, ref.cols])
    assert r64 <= 1.0, r64
    zs = er.natural_zs(n, m1 - 1, R)
    Fb = er.blocked_eval(funcs, X, zs=zs)
    rl, rd = ref.ratios(Fb, er.max_violation(Fb, ref.relops))
    print('%s: float64 tier / bound %.2e; blocked reversed order (zs = %d) / bound: %.2e (longdouble tier), %.2e (float64 tier)' % (shape, r64, zs, rl, rd))
    assert rl <= 1.0 and rd <= 1.0, (rl, rd)
    assert ref.accepts(ref.F64, ref.mv64)


@pytest.mark.parametrize('shape', TRIAL_SHAPES[1:])
def test_a_single_deleted_term_is_refused(trial, shape):
    funcs, X, ref = trial[shape]
    rs = np.random.RandomState(5)
    n = X.shape[0]
    for _ in range(8):
        k, c = int(rs.randint(len(funcs) - 1)), int(ref.cols[rs.randint(ref.cols.size)])      # (the last function is the ball: diagonal)
        i = int(rs.randint(n))
        j = (i + 1 + int(rs.randint(n - 1))) % n
        P = er.dense_of(ref.funcs[k][0])
        F = ref.F64.copy()
        F[k, c] -= P[i, j] * X[i, c] * X[j, c]          # ONE of the two symmetric off-diagonal terms
        assert not ref.accepts(F), (shape, k, c, i, j)


def eval_mutants(funcs, X, ref, zs):
    """name -> (F, maxviol) of host-made wrong evaluations."""
    good = er.blocked_eval(funcs, X, zs=zs)
    assert ref.accepts(good, er.max_violation(good, ref.relops))          # the twin itself is right
    out = {}
    for name, kw in (('last row block dropped', dict(drop_last_block=True)), ('last K-slice plane dropped', dict(drop_last_plane=True)),
                     ('r_k added once per plane', dict(r_per_plane=True)), ('padding rows filled with ones', dict(pad_ones=True))):
        if (name.startswith('padding') and X.shape[0] % 16 == 0) or ('plane' in name and zs == 1):
            continue
        F = er.blocked_eval(funcs, X, zs=zs, **kw)
        out[name] = (F, er.max_violation(F, ref.relops))
    if X.shape[1] > 1:
        F = good.copy()
        c = min(17, X.shape[1] - 2)
        F[:, c] = good[:, c + 1]
        out['one column taken from its neighbour'] = (F, er.max_violation(F, ref.relops))
    if '==' in ref.relops:
        out["'==' scored as '<='"] = (good, er.max_violation(good, [None] + ['<='] * (len(funcs) - 1)))
    return out


@pytest.mark.parametrize('table,case', [('3a', (100, 7, 112)), ('3a debug', (17, 4, 17)), ('3b', (130, 200)), ('3c', (17, 4, 16))])
def test_wrong_evaluations_are_refused(table, case):
    if table == '3b':
        n, R = case
        funcs, path, zs = er.sep_family('bls', n, seed=2), 'sep', 2       # two row-block groups: two partial planes per wave row
    elif table == '3c':
        n, m, R = case
        funcs, path, zs = er.coupled_problem(n, m, seed=n + m), 'coo', 1
    else:
        n, m, R = case
        funcs, path, zs = er.coupled_problem(n, m, seed=n + m), 'dense', 3 if n > 64 else 2
    X = er.population(n, R, seed=n + R)
    ref = er.Reference(funcs, X, er.eval_K(funcs, path), seed=R)
    muts = eval_mutants(funcs, X, ref, zs)
    need = {'one column taken from its neighbour', "'==' scored as '<='", 'last row block dropped'}
    if zs > 1:
        need |= {'last K-slice plane dropped', 'r_k added once per plane'}
    if n % 16:
        need.add('padding rows filled with ones')
    assert need <= set(muts), (need, sorted(muts))
    for name, (F, mv) in muts.items():
        assert not ref.accepts(F, mv), (table, case, name)


def test_wrong_products_are_refused():
    """weighted_matrix, weighted_product and sdr_sample: the unsymmetrised matrix, a dropped row block, a neighbour's column,
    a missing mean."""
    n, m, R = 100, 7, 47
    funcs = er.coupled_problem(n, m, seed=3)
    X = er.population(n, R, seed=4)
    rs = np.random.RandomState(6)
    w = rs.randn(m + 1)
    S, M = er.weighted_sum_ld(funcs, w)
    S64 = S.astype(np.float64)
    assert er.worst_ratio(S64, S, er.wmat_bound(m, M)) <= 1.0
    raw = sum(wk * er.dense_of(f[0]) for wk, f in zip(w, funcs))          # NOT symmetrised: the skew parts are still in
    assert er.worst_ratio(raw, S, er.wmat_bound(m, M)) > 1.0
    T = S64.copy()
    T[3, 70] = T[70, 3] * (1.0 + 2.0 ** -40)                                # one entry of the transpose, a few thousand ulps off
    assert er.worst_ratio(T, S, er.wmat_bound(m, M)) > 1.0
    ref, bound = er.wprod_reference(funcs, w, X)
    Y = S64 @ X
    assert er.worst_ratio(Y, ref, bound) <= 1.0
    assert er.worst_ratio(raw @ X, ref, bound) > 1.0                        # unsymmetrised P
    Z = Y.copy(); Z[96:] = 0.0
    assert er.worst_ratio(Z, ref, bound) > 1.0                              # last row block dropped
    Z = Y.copy(); Z[:, 17] = Y[:, 18]
    assert er.worst_ratio(Z, ref, bound) > 1.0                              # one column taken from its neighbour
    # sdr_sample
    n, S_ = 113, 113
    Fm, mu, Xi = rs.randn(n, n) / np.sqrt(n), rs.randn(n), rs.randn(n, S_)
    ref, bound = er.sample_reference(mu, Fm, Xi)
    Xs = mu[:, None] + Fm @ Xi
    assert er.worst_ratio(Xs, ref, bound) <= 1.0
    assert er.worst_ratio(Fm @ Xi, ref, bound) > 1.0                        # mean left out
    Z = Xs.copy(); Z[112:] = mu[112:, None]
    assert er.worst_ratio(Z, ref, bound) > 1.0                              # last row block of F dropped
    Z = Xs.copy(); Z[:, 111] = Xs[:, 112]
    assert er.worst_ratio(Z, ref, bound) > 1.0
    assert er.worst_ratio(mu[:, None] + Fm.T @ Xi, ref, bound) > 1.0        # transposed factor


def test_natural_k_splits_are_one_to_seven():
    got = [er.natural_zs(*shape) for shape, _ in er.NATURAL_ZS_CASES]
    assert got == [zs for _, zs in er.NATURAL_ZS_CASES] == [1, 2, 3, 4, 5, 6, 7], got
    # the splits the tables' other cases take: documented in profiles/r12_eval_domain.md
    for n, m, R in er.COUPLED_CASES + [er.FORCED_ZS_CASE] + er.DEBUG_DENSE_CASES:
        assert 1 <= er.natural_zs(n, m, R) <= min(7, er.n16_of(n) // 16)


def test_case_tables_sit_on_both_sides_of_the_thresholds():
    planes = {c: er.sep_takes_planes(*c) for c in er.SEP_CASES}
    assert not planes[(112, 200)] and not planes[(113, 112)] and planes[(113, 113)] and planes[(130, 200)] and not planes[(272, 100)]
    assert planes[(128, 128)] and planes[(257, 129)] and not planes[(320, 96)] and not planes[(64, 100)]
    for n, S in er.SAMPLE_CASES:
        assert er.sep_takes_planes(n, S) == ((n, S) == (113, 113))
