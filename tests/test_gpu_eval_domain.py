"""The evaluation and product operators over their dispatch domain, through the C ABI (Engine), against the plain high-precision
reference and the DERIVED bounds of tests/eval_reference.py (K u A, not 1e-12 (1 + |f|)):

  a  coupled constraints: dense_products_kernel<1> + dense_linear_kernel + dense_viol_kernel -- function groups, tile groups, the
     narrow arrangement, every K-split 1..7 (natural and forced), the dense path at n <= 64
  b  separable constraints: eval_kernel's per-tile MFMA loop on both sides of the switch to the planes path (MODE 2), four families
  c  the COO loop of eval_kernel (non-separable, n <= 64)
  d  eval_parts     e  weighted_matrix (and dense_gen_pack_kernel)     f  weighted_product     g  sdr_sample with given normals
  h  select_best with ties, worse buckets and bucket edges at R up to 2500
  i  state and isolation: a smaller population after a larger one, one non-finite column
  j  the K-split of CD's products (MODE 0), teacher-forced along the oracle's states

Every evaluation also asserts f0 == F[0] and maxviol == the maximum violation of the device's own F, bit for bit.
The worst error / bound of every group is printed (pytest -s) as 'eval-domain ratio <group> ...': profiles/r12_eval_domain.md."""
import numpy as np
import pytest
import scipy.sparse as sp

import eval_reference as er

pytestmark = pytest.mark.gpu

DENSE_PATH = 32 << 4   # qcqpmi_debug_profile switch: take the dense path on small problems too (default: n > 64)


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, funcs, dense_debug=False):
    from qcqp_amd.form import QCQPForm
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    if dense_debug:
        e.L.qcqpmi_debug_profile(e.h, DENSE_PATH, None)
    return e


def note(group, what, *ratios):
    print('eval-domain ratio %s %s: %s' % (group, what, ' '.join('%.3e' % r for r in ratios)))


def check_eval(e, ref, group, what):
    """eval() of the resident population against the reference; returns (f0, maxviol, F)."""
    f0, mv, F = e.eval(want_F=True)
    assert F.shape == ref.F64.shape
    assert er.same_bits(f0, F[0]), (group, what)
    assert er.same_bits(mv, er.device_max_violation(F, ref.relops)), (group, what)
    g0, gv = e.eval()                      # without the table of function values: the same numbers
    assert er.same_bits(g0, f0) and er.same_bits(gv, mv), (group, what)
    rl, rd = ref.ratios(F, mv)
    note(group, what, rl, rd)
    assert rl <= 1.0, (group, what, rl)     # against the longdouble tier: K u A
    assert rd <= 1.0, (group, what, rd)     # against the float64 tier: 2 K u A
    return f0, mv, F


# =============================================================================================== a. coupled constraints
def coupled_case(eng_mod, n, m, R, group, dense_debug=False):
    funcs = er.coupled_problem(n, m, seed=n + m)
    X = er.population(n, R, seed=n + R)
    ref = er.Reference(funcs, X, er.eval_K(funcs, 'dense'), seed=R)
    e = make(eng_mod, funcs, dense_debug)
    assert not e.separable
    e.upload(X)
    out = check_eval(e, ref, group, '(%d, %d, %d) zs=%d' % (n, m, R, er.natural_zs(n, m, R)))
    e.close()
    return out


@pytest.mark.parametrize('n,m,R', er.COUPLED_CASES)
def test_coupled_eval_over_groups_and_arrangements(eng_mod, n, m, R):
    coupled_case(eng_mod, n, m, R, 'a')


@pytest.mark.parametrize('n,m,R,zs', [c + (z,) for c, z in er.NATURAL_ZS_CASES if c not in er.COUPLED_CASES])
def test_coupled_eval_at_every_natural_k_split(eng_mod, n, m, R, zs):
    """The shapes whose natural split is 1, 2, 3, 4 (5, 6, 7 are cases of the table above)."""
    assert er.natural_zs(n, m, R) == zs
    coupled_case(eng_mod, n, m, R, 'a')


def test_coupled_eval_forced_k_splits_agree(eng_mod, monkeypatch):
    n, m, R = er.FORCED_ZS_CASE
    funcs = er.coupled_problem(n, m, seed=n + m)
    X = er.population(n, R, seed=n + R)
    ref = er.Reference(funcs, X, er.eval_K(funcs, 'dense'), seed=R)
    e = make(eng_mod, funcs)
    e.upload(X)
    Fs = []
    for zs in range(1, 8):
        monkeypatch.setenv('QCQPMI_DENSE_ZS', str(zs))
        Fs.append(check_eval(e, ref, 'a', '(%d, %d, %d) forced zs=%d' % (n, m, R, zs))[2])
    monkeypatch.delenv('QCQPMI_DENSE_ZS')
    for a in range(7):
        for b in range(a + 1, 7):
            assert np.all(np.abs(Fs[a] - Fs[b]) <= 2.0 * ref.bound), (a + 1, b + 1)
    assert any(not er.same_bits(Fs[0], F) for F in Fs[1:])       # the splits are different orders of summation: the switch acts
    e.close()


@pytest.mark.parametrize('n,m,R', er.DEBUG_DENSE_CASES)
def test_coupled_eval_dense_path_at_small_n(eng_mod, n, m, R):
    coupled_case(eng_mod, n, m, R, 'a', dense_debug=True)


def test_coupled_eval_exact_values(eng_mod):
    """x = 0 returns r_k bit for bit; a population inside every '<=' constraint returns maxviol == +0.0."""
    from qcqp_amd import problems
    n, m, R = 100, 9, 40
    funcs = er.coupled_problem(n, m, seed=2)
    X = er.population(n, R, seed=3)
    X[:, [0, 17, R - 1]] = 0.0
    e = make(eng_mod, funcs)
    e.upload(X)
    f0, mv, F = e.eval(want_F=True)
    rk = np.array([f[2] for f in funcs])
    for c in (0, 17, R - 1):
        assert er.same_bits(F[:, c], rk), c
    e.close()
    funcs = problems.dense_indefinite(n, m, seed=4)[0]            # every constraint a '<=' with r_k < 0
    assert all(f[3] == '<=' and f[2] < 0 for f in funcs[1:])
    X = 0.01 * np.random.RandomState(5).randn(n, R)
    ref = er.Reference(funcs, X, er.eval_K(funcs, 'dense'))
    assert np.all(ref.F64[1:] + 2 * ref.bound[1:] < 0)           # feasible beyond doubt
    e = make(eng_mod, funcs)
    e.upload(X)
    f0, mv, F = check_eval(e, ref, 'a', 'feasible (%d, %d, %d)' % (n, m, R))
    assert er.same_bits(mv, np.zeros(R)), mv                      # +0.0: not -inf, not -0.0, not negative
    e.close()


# ============================================================================================= b. separable constraints
def boundary_columns(X, seed):
    """Overwrite up to three columns with feasible-boundary points x_i = +-(1 + k 2^-52), k a small integer: f_k = x_i^2 - 1 is a
    few ulps of 1 there, far below 1e-12 (1 + |f|) -- and the terms that produce it are not."""
    n, R = X.shape
    rs = np.random.RandomState(seed)
    cols = sorted({R - 1} | ({1} if R > 2 else set()) | ({R // 2} if R > 4 else set()))
    for c in cols:
        X[:, c] = rs.choice([-1.0, 1.0], size=n) * (1.0 + rs.randint(-3, 4, size=n) * 2.0 ** -52)
    return cols


@pytest.mark.parametrize('family', er.SEP_FAMILIES)
@pytest.mark.parametrize('n,R', er.SEP_CASES)
def test_separable_eval_both_sides_of_the_planes_switch(eng_mod, n, R, family):
    funcs = er.sep_family(family, n, seed=n % 7 + 1)
    X = er.population(n, R, seed=n + R)
    bcols = boundary_columns(X, seed=R)
    ref = er.Reference(funcs, X, er.eval_K(funcs, 'sep'), seed=R)
    e = make(eng_mod, funcs)
    assert e.separable
    e.upload(X)
    f0, mv, F = check_eval(e, ref, 'b', '%s (%d, %d) %s' % (family, n, R, 'planes' if er.sep_takes_planes(n, R) else 'per-tile'))
    # the order of the rows of F is the function index: row k holds the constraint on ITS coordinate
    fs = ref.funcs
    for k in (1, len(fs) // 2, len(fs) - 1):
        i = int(sp.coo_matrix(fs[k][0]).row[0]) if sp.coo_matrix(fs[k][0]).nnz else int(np.nonzero(fs[k][1])[0][0])
        p, q, r = float(er.dense_of(fs[k][0])[i, i]), float(fs[k][1][i]), fs[k][2]
        assert np.all(np.abs(F[k] - ((p * X[i] + q) * X[i] + r)) <= 2 * er.K_SEP * er.U * (abs(p) * X[i] ** 2 + abs(q * X[i]) + abs(r))), k
    if family in ('bls', 'cut'):
        # the boundary columns: |f_k| is a few ulps of 1, and what separates a right value from a wrong one is the bound
        assert np.all(np.abs(F[1:, bcols]) <= 16 * 2.0 ** -52)
        assert np.all(ref.bound[1:, bcols] <= 16 * er.U)
    e.close()


# ========================================================================================================== c. COO loop
@pytest.mark.parametrize('R', er.COO_RS)
@pytest.mark.parametrize('n,m', er.COO_CASES)
def test_coo_eval_small_coupled_problems(eng_mod, n, m, R):
    funcs = er.coupled_problem(n, m, seed=n + m, csr=False)
    allcsr = [(sp.csr_matrix(P), q, r, rel) for P, q, r, rel in funcs]
    X = er.population(n, R, seed=n + R)
    ref = er.Reference(funcs, X, er.eval_K(funcs, 'coo'), seed=R)
    outs = []
    for name, fs in (('dense', funcs), ('csr', allcsr)):
        e = make(eng_mod, fs)
        assert not e.separable
        e.upload(X)
        outs.append(check_eval(e, ref, 'c', '%s (%d, %d, %d)' % (name, n, m, R)))
        e.close()
    for a, b in zip(outs[0], outs[1]):
        assert er.same_bits(a, b)            # the two uploads hold the same entries in the same order


# ========================================================================================================= d. eval_parts
@pytest.mark.parametrize('n,m,R', er.PARTS_CASES)
def test_eval_parts_against_the_two_halves(eng_mod, n, m, R):
    funcs = er.coupled_problem(n, m, seed=n + m)
    X = er.population(n, R, seed=n + R)
    Z = sp.csr_matrix((n, n))
    K = er.K_dense(n)
    ref = er.Reference(funcs, X, K, seed=R)
    refq = er.Reference([(P, 0 * q, r, rel) for P, q, r, rel in funcs], X, K, seed=R)
    refl = er.Reference([(Z, q, 0.0, rel) for P, q, r, rel in funcs], X, er.n16_of(n) + 2, seed=R)
    e = make(eng_mod, funcs)
    e.upload(X)
    before = e.eval(want_F=True)
    quad, lin = e.eval_parts()
    rq, rl = refq.ratios(quad), refl.ratios(lin)
    note('d', '(%d, %d, %d) zs=%d quad' % (n, m, R, er.natural_zs(n, m, R)), *rq)
    note('d', '(%d, %d, %d) lin' % (n, m, R), *rl)
    assert max(rq) <= 1.0 and max(rl) <= 1.0, (rq, rl)
    assert np.all(np.abs(quad + lin - before[2]) <= refq.bound + refl.bound)
    after = e.eval(want_F=True)
    for a, b in zip(before, after):
        assert er.same_bits(a, b)            # eval_parts leaves nothing behind that the next evaluation reads
    check_eval(e, ref, 'd', '(%d, %d, %d) eval after parts' % (n, m, R))
    e.close()


# ==================================================================================================== e. weighted_matrix
@pytest.mark.parametrize('n,debug', [(n, False) for n in er.WMAT_NS] + [(n, True) for n in er.WMAT_DEBUG_NS])
def test_weighted_matrix(eng_mod, n, debug):
    m = 6
    funcs = er.coupled_problem(n, m, seed=n + m)                 # dense uploads and one CSR upload (function 3)
    assert sp.issparse(funcs[3][0]) and not sp.issparse(funcs[2][0])
    fs = er.symmetrised(funcs)
    e = make(eng_mod, funcs, debug)
    for k in range(m + 1):
        w = np.zeros(m + 1)
        w[k] = 1.0
        S = e.weighted_matrix(w)
        assert er.same_bits(S, er.dense_of(fs[k][0]) + 0.0), k     # w = e_k: the uploaded (symmetrised) matrix itself
    w = np.zeros(m + 1)
    w[2], w[5] = 8.0, -0.25                                          # powers of two on an even and an odd index: one rounding
    assert er.same_bits(e.weighted_matrix(w), 8.0 * er.dense_of(fs[2][0]) + (-0.25) * er.dense_of(fs[5][0]))
    rs = np.random.RandomState(n)
    worst = 0.0
    for trial in range(3):
        w = rs.randn(m + 1) * 10.0 ** rs.uniform(-2, 2, size=m + 1)
        w[rs.randint(m + 1)] = 0.0
        w[rs.randint(m + 1)] *= -1.0
        if trial == 2:
            w[1:] = np.where(np.arange(1, m + 1) % 2 == 0, 0.0, -np.abs(w[1:]))      # zeros on every even function
        S = e.weighted_matrix(w)
        assert er.same_bits(S, S.T)
        Sld, M = er.weighted_sum_ld(funcs, w)
        worst = max(worst, er.worst_ratio(S, Sld, er.wmat_bound(m, M)))
    note('e', 'n=%d' % n, worst)
    assert worst <= 1.0, worst
    e.close()


def test_generated_functions_through_weighted_matrix(eng_mod):
    """dense_gen_pack_kernel without a host twin: every P_k of a generated form is downloaded with w = e_k, and eval() of the
    generated context is checked against the reference built from those matrices and linear_terms()."""
    from qcqp_amd import problems
    n, m, R = 100, 5, 48
    form = problems.dense_indefinite_generated(n, m, seed=9)
    e = eng_mod.Engine(form)
    Q, r, rel = e.linear_terms()
    funcs = []
    for k in range(m + 1):
        w = np.zeros(m + 1)
        w[k] = 1.0
        P = e.weighted_matrix(w)
        assert er.same_bits(P, P.T), k
        funcs.append((P, Q[k], float(r[k]), rel[k]))
    assert np.array_equal(funcs[m][0], np.eye(n))                      # the ball
    for k in range(m):
        assert np.count_nonzero(funcs[k][0]) == n * n and abs(np.std(funcs[k][0]) * np.sqrt(2.0 * n) - 1.0) < 0.1, k     # N(0, 1/2n) off the diagonal
        assert not np.array_equal(funcs[k][0], funcs[(k + 1) % m][0])
    X = er.population(n, R, seed=10)
    ref = er.Reference(funcs, X, er.eval_K(funcs, 'dense'), seed=R)
    e.upload(X)
    check_eval(e, ref, 'e', 'generated (%d, %d, %d)' % (n, m, R))
    e.close()


# =================================================================================================== f. weighted_product
def wprod_case(e, funcs, used, n, rs, group_note):
    """used: how many leading functions take part (all of them, or the objective alone on a separable context)."""
    m = len(funcs) - 1
    worst = 0.0
    for R in er.WPROD_RS:
        X = er.population(n, R, seed=n + R)
        e.upload(X)
        ws = [np.eye(m + 1)[0], rs.randn(m + 1) * 10.0 ** rs.uniform(-2, 2, size=m + 1)]
        w = -np.abs(rs.randn(m + 1))
        w[1::2] = 0.0
        ws.append(w)
        for w in ws:
            Y = e.weighted_product(w)
            assert Y.shape == (n, R)
            wu = np.where(np.arange(m + 1) < used, w, 0.0)
            ref, bound = er.wprod_reference(funcs, wu, X)
            worst = max(worst, er.worst_ratio(Y, ref, bound))
            assert er.worst_ratio(Y, ref, bound) <= 1.0, (n, R, w[:3])
        # w = e_0 against NumPy's own product
        P0 = er.dense_of(er.symmetrised(funcs)[0][0])
        Y = e.weighted_product(ws[0])
        assert np.all(np.abs(Y - P0 @ X) <= 2.0 * (er.n16_of(n) + m + 5) * er.U * (np.abs(P0) @ np.abs(X))), (n, R)
    note('f', group_note, worst)


@pytest.mark.parametrize('n', er.WPROD_COUPLED_NS)
def test_weighted_product_coupled(eng_mod, n):
    m = 6
    funcs = er.coupled_problem(n, m, seed=n + m)
    e = make(eng_mod, funcs)
    wprod_case(e, funcs, m + 1, n, np.random.RandomState(n), 'coupled n=%d' % n)
    e.close()


@pytest.mark.parametrize('n', er.WPROD_SEP_NS)
def test_weighted_product_separable(eng_mod, n):
    funcs = er.sep_family('boxz', n, seed=3)
    e = make(eng_mod, funcs)
    assert e.separable
    wprod_case(e, funcs, 1, n, np.random.RandomState(n), 'separable n=%d' % n)       # Y = w_0 P0 X
    e.close()


# ========================================================================================================= g. sdr_sample
@pytest.mark.parametrize('n', sorted({c[0] for c in er.SAMPLE_CASES}))
def test_sdr_sample_with_given_normals(eng_mod, n):
    from qcqp_amd import problems
    Ss = [S for nn, S in er.SAMPLE_CASES if nn == n]
    rs = np.random.RandomState(n)
    Fm = rs.randn(n, n) / np.sqrt(n) * 10.0 ** rs.uniform(-1, 1, size=(n, 1))
    mu = rs.randn(n) * 10.0 ** rs.uniform(-2, 2, size=n)
    Xi = rs.randn(n, max(Ss))
    e = make(eng_mod, problems.maxcut(n, seed=2, weighted=True)[0])
    got = {}
    for S in Ss:
        e.sdr_sample(mu, Fm, S, Xi=Xi[:, :S])
        X = e.download()
        ref, bound = er.sample_reference(mu, Fm, Xi[:, :S])
        ratio = er.worst_ratio(X, ref, bound)
        note('g', '(%d, %d) %s' % (n, S, 'MODE 3' if er.sep_takes_planes(n, S) else 'affine_tiles'), ratio)
        assert ratio <= 1.0, (n, S, ratio)
        got[S] = (X, bound)
    Smin = min(Ss)
    for S in Ss:         # the same samples through the other kernel (n = 113: S = 112 affine_tiles_kernel, S = 113 MODE 3)
        assert np.all(np.abs(got[S][0][:, :Smin] - got[Smin][0]) <= 2.0 * got[Smin][1]), (n, S)
    e.close()


# ======================================================================================================== h. select_best
TOL = 1e-4


def select_population(funcs, kind, n, R, seed):
    """Columns in bucket 0 (several of them copies of one another and of the best of them), columns with a lower objective in a
    worse bucket, columns on a bucket edge (maxviol = 2 tol up to rounding)."""
    rs = np.random.RandomState(seed)
    fs = er.symmetrised(funcs)
    P0, q0 = er.dense_of(fs[0][0]), fs[0][1]
    if kind == 'sep':        # x_i^2 == 1
        X = rs.choice([-1.0, 1.0], size=(n, R))
    else:                    # ball ||x||^2 <= n
        X = rs.randn(n, R) * rs.uniform(0.1, 0.9, size=R)
    f = np.einsum('ir,ir->r', X, P0 @ X) + q0 @ X
    if kind != 'sep':
        f = np.where(np.einsum('ir,ir->r', X, X) < 0.999 * n, f, np.inf)      # the best of the columns inside the ball
    best = int(np.argmin(f))
    x = X[:, best].copy()
    spots = sorted({R // 3, (R // 3 + 1024) % R, R - 1, (best + 1) % R})      # same thread (r + 1024), other threads, the last column
    for c in spots:
        X[:, c] = x                                                            # exact ties of (bucket, f0)
    free = [c for c in range(R) if c not in spots and c != best]
    if len(free) >= 4:
        g = 2.0 * P0 @ x + q0
        i = int(np.argmax(np.abs(g)))
        lam, V = np.linalg.eigh(P0)
        for j, c in enumerate(free[:2]):      # a lower objective in a worse bucket
            y = x.copy()
            if kind == 'sep':                 # a step towards the minimiser along coordinate i: f0 falls, x_i^2 leaves 1
                y[i] = x[i] - np.sign(g[i]) * (abs(g[i]) / (2.0 * P0[i, i])) * (1.0 - 0.25 * j)
            else:                             # outside the ball along the most negative curvature of the objective
                y = np.sqrt(n + 1.0 + j) * V[:, 0] * (-1.0 if float(q0 @ V[:, 0]) > 0 else 1.0)
            X[:, c] = y
        for j, c in enumerate(free[2:4]):     # bucket edge: violation = 2 tol up to rounding
            y = x.copy()
            if kind == 'sep':
                y[j] = np.sign(x[j]) * np.sqrt(1.0 + 2.0 * TOL)
            else:
                y = x * np.sqrt((n + 2.0 * TOL) / float(x @ x))
            X[:, c] = y
    return X


@pytest.mark.parametrize('R', er.SELECT_RS)
@pytest.mark.parametrize('kind', ['sep', 'coupled'])
def test_select_best_ties_buckets_and_edges(eng_mod, kind, R):
    from qcqp_amd import dist, problems
    n = 40 if kind == 'sep' else 65
    funcs = problems.boolean_least_squares(n, 60, seed=5)[0] if kind == 'sep' else problems.dense_indefinite(n, 1, seed=6)[0]
    X = select_population(funcs, kind, n, R, seed=R)
    ref = er.Reference(funcs, X, er.eval_K(funcs, 'sep' if kind == 'sep' else 'dense'), seed=R)
    e = make(eng_mod, funcs)
    assert e.separable == (kind == 'sep')
    e.upload(X)
    f0, mv, F = check_eval(e, ref, 'h', '%s R=%d' % (kind, R))
    idx, fb, vb, xb = e.select_best(tol=TOL)
    want = dist.select_best_host(f0, mv, tol=TOL)
    assert idx == want[2], (idx, want)
    assert er.same_bits(fb, f0[idx]) and er.same_bits(vb, mv[idx]) and er.same_bits(xb, X[:, idx])
    # the population holds what it is meant to hold (by the reference)
    rb = np.floor(ref.mv64 / TOL)
    wr = dist.select_best_host(ref.F64[0], ref.mv64, tol=TOL)
    if R >= 15:
        assert int(np.sum(np.all(X == X[:, [wr[2]]], axis=0))) >= 3                          # exact ties with the winner
        assert np.any((rb > wr[0]) & (ref.F64[0] + 2 * ref.bound[0] < wr[1]))                 # lower objective, worse bucket
        assert np.any(np.floor((ref.mv64 - 2 * ref.mv_bound) / TOL) != np.floor((ref.mv64 + 2 * ref.mv_bound) / TOL))      # on an edge
    # the reference's winner, wherever its buckets and objectives decide beyond the bound
    lo, hi = np.floor(np.maximum(ref.mv64 - 2 * ref.mv_bound, 0.0) / TOL), np.floor((ref.mv64 + 2 * ref.mv_bound) / TOL)      # (a violation is >= 0)
    rivals = (lo <= wr[0]) & ~np.all(X == X[:, [wr[2]]], axis=0)
    decided = lo[wr[2]] == hi[wr[2]] and np.all((lo[rivals] == hi[rivals]) & (lo[rivals] == wr[0])) and \
        np.all(ref.F64[0][rivals] - 2 * ref.bound[0][rivals] > wr[1] + 2 * ref.bound[0][wr[2]])
    print('eval-domain select %s R=%d: winner %d, reference winner decided beyond the bound: %s' % (kind, R, idx, bool(decided)))
    assert decided
    # (copies of one column are exact ties on the device; the float64 tier's BLAS rounds a column by its position in the matrix,
    # so among the copies the reference's own order is noise: the lowest index of them wins)
    assert idx == int(np.flatnonzero(np.all(X == X[:, [wr[2]]], axis=0))[0]), (idx, wr)
    e.close()


# ================================================================================================ i. state and isolation
def path_context(eng_mod, path):
    """(engine, funcs, n, term counts, operator) of one context per path."""
    if path == 'planes':
        funcs, n, kp = er.sep_family('bls', 130, seed=3), 130, 'sep'
    elif path == 'per-tile':
        funcs, n, kp = er.sep_family('bls', 112, seed=3), 112, 'sep'
    else:
        funcs, n, kp = er.coupled_problem(100, 7, seed=3), 100, 'dense'
    return make(eng_mod, funcs), funcs, n, kp


def run_op(e, path):
    if path == 'weighted_product':
        w = np.linspace(-1.0, 2.0, e.m + 1)
        return (e.weighted_product(w),)
    return e.eval(want_F=True)


@pytest.mark.parametrize('path', ['planes', 'per-tile', 'coupled', 'weighted_product'])
def test_a_smaller_population_after_a_larger_one(eng_mod, path):
    e, funcs, n, kp = path_context(eng_mod, path)
    big = 1e6 * np.random.RandomState(1).randn(n, 208)
    small = er.population(n, 17, seed=2)
    e.upload(big)
    run_op(e, path)
    if path == 'planes':
        assert er.sep_takes_planes(n, 208)
    e.upload(small)
    got = run_op(e, path)
    fresh, _, _, _ = path_context(eng_mod, path)
    fresh.upload(small)
    want = run_op(fresh, path)
    for a, b in zip(got, want):
        assert er.same_bits(a, b)
    e.close()
    fresh.close()


@pytest.mark.parametrize('bad', [np.inf, np.nan])
@pytest.mark.parametrize('path', ['planes', 'per-tile', 'coupled', 'weighted_product'])
def test_one_non_finite_column_stays_alone(eng_mod, path, bad):
    e, funcs, n, kp = path_context(eng_mod, path)
    R, c, i = 208, 77, n - 3
    X = er.population(n, R, seed=4)
    e.upload(X)
    clean = run_op(e, path)
    Xb = X.copy()
    Xb[i, c] = bad
    e.upload(Xb)
    dirty = run_op(e, path)
    others = np.arange(R) != c
    for a, b in zip(clean, dirty):
        assert er.same_bits(a[..., others], b[..., others])
    assert not np.isfinite(dirty[0][..., c]).all()                   # f0 (or the product's column) of that column
    if path != 'weighted_product':
        assert not np.isfinite(dirty[0][c])
    e.upload(X)                                                      # and nothing of it stays behind
    for a, b in zip(clean, run_op(e, path)):
        assert er.same_bits(a, b)
    e.close()


# ================================================================================ j. K-split of CD's products, teacher-forced
@pytest.fixture(scope='module')
def cd_oracle_walk(orc):
    """The oracle's states around blocks 0 and 6 (ragged: 4 coordinates) of sweep 0 of phase 1: per block, the state before its
    first visit and the value every visit writes, for every restart."""
    from qcqp_amd import problems
    n, R, seed, first = 100, 32, 13, 5
    funcs = problems.dense_indefinite(100, 30, seed=11)[0]
    prob = orc.Problem(funcs)
    X0 = 1.5 * np.random.RandomState(3).randn(n, R)

    def visits(x, r, i0, cnt):
        rng = orc.Rng(orc.RNG_KEYED, seed)
        rng.set_restart(first + r)
        return prob.cd_visits(1, x, 0, i0, cnt, rng=rng)
    walk = {}
    # (block, from X0 directly): by block 6 of the oracle's own sweep every restart is feasible and its four visits move nothing --
    # the engine must not move either --, so the ragged block is ALSO walked from X0, where its visits do move
    for b, cnt, direct in ((0, 16, True), (6, 4, False), (6, 4, True)):
        start = np.stack([X0[:, r].copy() if direct else visits(X0[:, r], r, 0, 16 * b) for r in range(R)], axis=1)
        after = np.empty((cnt, R))
        cur = start.copy()
        for c in range(cnt):
            for r in range(R):
                cur[:, r] = visits(cur[:, r], r, 16 * b + c, 1)
                after[c, r] = cur[16 * b + c, r]
        walk[(b, direct)] = (start, after)
    return funcs, seed, first, walk


@pytest.mark.parametrize('zs', range(1, 8))
def test_cd_products_k_split_teacher_forced(eng_mod, cd_oracle_walk, monkeypatch, zs):
    funcs, seed, first, walk = cd_oracle_walk
    monkeypatch.setenv('QCQPMI_DENSE_ZS', str(zs))
    e = make(eng_mod, funcs)
    worst = 0.0
    for (b, direct), (start, after) in sorted(walk.items()):
        cur = start.copy()
        for c in range(after.shape[0]):
            e.upload(cur)
            e.cd_dense_block_step(1, 0, b, seed=seed, first_index=first, coords=(c, c + 1))
            X1 = e.download()
            i = 16 * b + c
            d = np.abs(X1[i] - after[c]) / (1.0 + np.max(np.abs(cur), axis=0))
            worst = max(worst, float(d.max()))
            assert np.all(d <= 1e-8), (zs, b, c, float(d.max()))
            keep = np.arange(cur.shape[0]) != i
            assert np.array_equal(X1[keep], cur[keep])                 # one visit moves one coordinate
            cur[i] = after[c]
    assert e.last_cd_kernel() == 'dense_chain_mw_kernel'
    note('j', 'zs=%d worst relative distance from the oracle' % zs, worst)
    e.close()
