"""Synthetic QCQP generators (host side, NumPy only).

They mirror the problem families of the reference's examples and of
BASELINE.json's configs; each returns a list of ``(P, q, r, relop)`` tuples
with the objective first (relop ``None``) -- the raw-array form accepted by
``qcqp_amd.QCQPForm.from_arrays`` -- plus a ``maximize`` flag.

* ``boolean_least_squares``  -- examples/boolean_least_squares.py:6-15
* ``maxcut``                 -- examples/maxcut.py:9-21
* ``box_least_squares``      -- the box-constrained sibling of the Boolean family (one interval per coordinate)
* ``box_qp``                 -- the box-constrained QP with an INDEFINITE objective (a diagonal of mixed sign)
* ``boolean_least_squares_batch`` / ``box_qp_batch`` -- B small problems with shared constraints (qcqp_amd.batch.QCQPBatch)
* ``per_problem_constraints_batch`` -- B small problems with the same constraint STRUCTURE and their own coefficients
* ``beamforming``            -- examples/secondary_user_beamforming.py:18-41
* ``dense_indefinite``       -- SURVEY.md section 8(d) cfg5 generator
* ``circle_packing``         -- examples/circle_packing.py:6-17 (two variables: centres 2 x N and the radius)
"""
import numpy as np
import scipy.sparse as sp


def boolean_least_squares(n, m_rows, seed=1, legacy_seed=False):
    """minimize ||Ax-b||^2  s.t. x_i^2 == 1.

    legacy_seed=True draws A, b exactly like the example script
    (np.random.seed(seed); randn(m, n); randn(m, 1))."""
    if legacy_seed:
        st = np.random.get_state()
        np.random.seed(seed)
        A = np.random.randn(m_rows, n)
        b = np.random.randn(m_rows, 1)
        np.random.set_state(st)
    else:
        rs = np.random.RandomState(seed)
        A = rs.randn(m_rows, n)
        b = rs.randn(m_rows, 1)
    P0 = A.T.dot(A)
    P0 = (P0 + P0.T) / 2.
    q0 = (-2. * A.T.dot(b)).ravel()
    r0 = float(b.T.dot(b)[0, 0])
    funcs = [(P0, q0, r0, None)]
    for i in range(n):
        P = sp.csr_matrix(([1.0], ([i], [i])), shape=(n, n))
        funcs.append((P, np.zeros(n), -1.0, '=='))
    return funcs, False, dict(A=A, b=b)


def box_least_squares(n, m_rows, bound=1.0, seed=1, ridge=0.1):
    """minimize ||Ax-b||^2 + ridge ||x||^2  s.t. x_i^2 <= bound^2  (the box -bound <= x_i <= bound as one convex quadratic per
    coordinate: ONE constraint class, one interval per coordinate -- the relaxed sibling of boolean_least_squares)."""
    rs = np.random.RandomState(seed)
    A = rs.randn(m_rows, n)
    b = rs.randn(m_rows, 1) * np.sqrt(n)
    P0 = A.T.dot(A) + ridge * np.eye(n)
    P0 = (P0 + P0.T) / 2.
    q0 = (-2. * A.T.dot(b)).ravel()
    r0 = float(b.T.dot(b)[0, 0])
    funcs = [(P0, q0, r0, None)]
    for i in range(n):
        P = sp.csr_matrix(([1.0], ([i], [i])), shape=(n, n))
        funcs.append((P, np.zeros(n), -float(bound) ** 2, '<='))
    return funcs, False, dict(A=A, b=b)


def box_qp(n, seed=1, lo=-1.0, hi=1.0, zero_every=0, density=1.0, relop='<=', diagonal=None):
    """minimize x^T P0 x + q0^T x  s.t. (x_i - lo)(x_i - hi) <= 0  -- the box-constrained QP with an indefinite objective, the
    textbook nonconvex QCQP.  P0 = (G + G^T) / 2 with G ~ N(0, 1): its diagonal is N(0, 1), about half of it negative; q0 =
    sqrt(n) N(0, 1) (the scale of a row of P0 times a point of the box).  ONE constraint class, one constraint per coordinate.
      zero_every = k > 0   every k-th diagonal entry of P0 (i = k - 1, 2 k - 1, ...) is set to 0: a diagonal of all three signs
      density < 1          every off-diagonal pair (i, j), (j, i) is kept with this probability (the diagonal always)
      relop = '=='         the two-interval sibling (x_i - lo)(x_i - hi) == 0, i.e. x_i in {lo, hi} (x_i^2 == 1 for the box
                           [-1, 1]): at the slack s phase 1 leaves, the feasible set is one interval around lo and one around hi
      diagonal             'negative': the diagonal is replaced by -|diagonal|, a concave scalar objective in every coordinate
                           (zero_every still applies); 'only': the off-diagonal part is dropped (every coordinate on its own)
    Returns (funcs, maximize, info) like the other generators; info['diag'] is the diagonal of P0."""
    rs = np.random.RandomState(seed)
    G = rs.randn(n, n)
    P0 = (G + G.T) / 2.
    q0 = np.sqrt(n) * rs.randn(n)
    if density < 1.0:
        keep = np.triu(rs.uniform(size=(n, n)) < density, 1)
        P0 = P0 * (keep + keep.T + np.eye(n, dtype=bool))
    d = np.diag(P0).copy()
    if diagonal == 'negative':
        d = -np.abs(d)
    elif diagonal == 'only':
        P0 = np.zeros((n, n))
    elif diagonal is not None:
        raise KeyError(diagonal)
    if zero_every > 0:
        d[zero_every - 1::zero_every] = 0.0
    P0[np.arange(n), np.arange(n)] = d
    funcs = [(P0, q0, 0.0, None)]
    for i in range(n):
        P = sp.csr_matrix(([1.0], ([i], [i])), shape=(n, n))
        qv = np.zeros(n)
        qv[i] = -(float(lo) + float(hi))
        funcs.append((P, qv, float(lo) * float(hi), relop))
    return funcs, False, dict(diag=d)


def boolean_least_squares_batch(B, n, m, seed=1, shared_A=False):
    """B Boolean least squares problems of n variables and m rows with the SAME constraints x_i^2 == 1 -- a frame of MIMO detection
    problems, one instance per subcarrier and symbol: minimize ||A_b x - b_b||^2.  Problem b draws (A_b, b_b) from
    RandomState(seed + b) in the order of boolean_least_squares, so problem b IS boolean_least_squares(n, m, seed + b);
    shared_A=True: one channel matrix A (that of problem 0) for the whole frame, only the received vectors b_b differ.
    Returns a list of B funcs lists (objective first) for qcqp_amd.batch.QCQPBatch; the constraint tuples are shared objects."""
    cons = boolean_least_squares(n, m, seed=seed)[0][1:]
    A0 = np.random.RandomState(seed).randn(m, n)
    out = []
    for b in range(int(B)):
        rs = np.random.RandomState(seed + b)
        A = rs.randn(m, n)
        bv = rs.randn(m, 1)
        if shared_A:
            A = A0
        P0 = A.T.dot(A)
        P0 = (P0 + P0.T) / 2.
        out.append([(P0, (-2. * A.T.dot(bv)).ravel(), float(bv.T.dot(bv)[0, 0]), None)] + cons)
    return out


def box_qp_batch(n, seeds, **kwargs):
    """The small-n variant of box_qp for a batch: problem b is box_qp(n, seed=seeds[b], **kwargs) -- its own indefinite objective --
    and all of them share the constraint tuples of the first (the constraints of box_qp do not depend on the seed).  Returns a
    list of funcs lists for qcqp_amd.batch.QCQPBatch."""
    seeds = [int(sd) for sd in np.atleast_1d(seeds)]
    cons = box_qp(n, seed=seeds[0], **kwargs)[0][1:]
    return [[box_qp(n, seed=sd, **kwargs)[0][0]] + cons for sd in seeds]


PER_PROBLEM_FAMILIES = ('boxpp', 'boxppneg', 'eq2pp', 'eqpp', 'annpp', 'linpp')


def per_problem_constraints_batch(name, n, seeds):
    """B = len(seeds) small problems whose constraints have the same STRUCTURE (number, touched coordinate, relop) and their own
    COEFFICIENTS -- what qcqp_amd.batch.QCQPBatch solves through qcqpmi_cd_small_batch_run_pc.  Problem b takes its objective from the
    shared-constraint generator at seed seeds[b] and draws its constraint coefficients from a RandomState keyed by (name, n,
    seeds[b]): it depends on seeds[b] alone, not on B or on its place in the list.
      boxpp     box_qp objective (indefinite diagonal); (x_i - lo)(x_i - hi) <= 0, lo ~ U(-2, 1), hi = lo + U(0.05, 2) per coordinate
      boxppneg  box_qp(diagonal='negative') objective; the same constraints
      eq2pp     box_qp objective; (x_i - lo)(x_i - hi) == 0, the same draws
      eqpp      Boolean least squares objective (n + n // 2 + 1 rows); x_i^2 == d, d ~ U(0.25, 4) (the unit-diagonal family of SDR)
      annpp     multi_class('ann2') objective; even i: x^2 <= ro^2 and -x^2 <= -ri^2, ro ~ U(0.8, 2), ri = ro U(0.2, 0.8);
                odd i: x^2 == U(0.25, 4)  (two constraints on a coordinate)
      linpp     box_qp objective; two LINEAR constraints per coordinate, x <= hi and -x <= -lo (p = 0), lo / hi as in boxpp
    Returns a list of funcs lists (objective first)."""
    import zlib
    if name not in PER_PROBLEM_FAMILIES:
        raise KeyError(name)
    key = zlib.crc32(name.encode())
    out = []
    for sd in [int(sd) for sd in np.atleast_1d(seeds)]:
        rs = np.random.RandomState([key, int(n), sd & 0xffffffff, (sd >> 32) & 0xffffffff])
        if name == 'boxppneg':
            funcs = [box_qp(n, seed=sd, diagonal='negative')[0][0]]
        elif name == 'eqpp':
            funcs = [boolean_least_squares(n, n + n // 2 + 1, seed=sd)[0][0]]
        elif name == 'annpp':
            funcs = [multi_class('ann2', n, seed=sd)[0]]
        else:
            funcs = [box_qp(n, seed=sd)[0][0]]

        def quad(i, p, q, r, relop):
            qv = np.zeros(n)
            qv[i] = float(q)
            funcs.append((sp.csr_matrix(([float(p)], ([i], [i])), shape=(n, n)), qv, float(r), relop))
        if name in ('boxpp', 'boxppneg', 'eq2pp', 'linpp'):
            lo = rs.uniform(-2.0, 1.0, size=n)
            hi = lo + rs.uniform(0.05, 2.0, size=n)
            for i in range(n):
                if name == 'linpp':
                    quad(i, 0.0, 1.0, -hi[i], '<=')
                    quad(i, 0.0, -1.0, lo[i], '<=')
                else:
                    quad(i, 1.0, -(lo[i] + hi[i]), lo[i] * hi[i], '==' if name == 'eq2pp' else '<=')
        elif name == 'eqpp':
            d = rs.uniform(0.25, 4.0, size=n)
            for i in range(n):
                quad(i, 1.0, 0.0, -d[i], '==')
        else:
            ro = rs.uniform(0.8, 2.0, size=n)
            ri = ro * rs.uniform(0.2, 0.8, size=n)
            d = rs.uniform(0.25, 4.0, size=n)
            for i in range(n):
                if i % 2 == 0:
                    quad(i, 1.0, 0.0, -ro[i] ** 2, '<=')
                    quad(i, -1.0, 0.0, ri[i] ** 2, '<=')
                else:
                    quad(i, 1.0, 0.0, -d[i], '==')
        out.append(funcs)
    return out


def multi_class(name, n, seed=1):
    """Separable problems with SEVERAL constraint classes and up to two constraints per coordinate (what cd_life_kernel's GENK / LINK
    kinds take; the reference treats every coordinate's list on its own, qcqp.py:113-141, 160-176).  Returns funcs (objective first).
      box3   least squares + ridge; coordinate i carries x^2 <= 1 | x^2 <= 0.49 | x^2 - x/2 - 1/2 <= 0 (= [-1/2, 1]) by i mod 3
      ann2   least squares + ridge; even i: x^2 <= 1 AND -x^2 <= -1/4 (two intervals [-1, -1/2] u [1/2, 1]); odd i: x^2 == 1
      lin2   least squares + ridge; TWO LINEAR constraints per coordinate, x <= u_c and -x <= -l_c, bounds by i mod 2
      cut2   weighted MAXCUT objective (zero diagonal); even i: x^2 == 1, odd i: x^2 <= 1 (a relaxed vertex)
      box4   least squares + ridge; FOUR classes by i mod 4 (the class table full): x^2 <= 1 | x^2 <= 0.49 | x^2 - x/2 - 1/2 <= 0 |
             the annulus pair x^2 <= 1 AND -x^2 <= -1/4
      cut4   weighted MAXCUT objective (zero diagonal); four classes by i mod 4: x^2 == 1 | x^2 <= 1 | x^2 <= 0.49 | the annulus pair"""
    rs = np.random.RandomState(seed)
    funcs = []
    if name in ('cut2', 'cut4'):
        U = np.triu((rs.uniform(size=(n, n)) < 0.5).astype(float), 1) * np.triu(rs.uniform(0.5, 1.5, size=(n, n)), 1)
        W = U + U.T
        funcs.append((0.25 * W, np.zeros(n), -0.25 * float(W.sum()), None))
    else:
        m_rows = max(4, n // 2)
        A = rs.randn(m_rows, n)
        b = rs.randn(m_rows, 1) * np.sqrt(n)
        P0 = A.T.dot(A) + 0.1 * np.eye(n)
        funcs.append(((P0 + P0.T) / 2., (-2. * A.T.dot(b)).ravel(), float(b.T.dot(b)[0, 0]), None))

    def quad(i, p, q, r, relop):
        P = sp.csr_matrix(([float(p)], ([i], [i])), shape=(n, n))
        qv = np.zeros(n)
        qv[i] = float(q)
        funcs.append((P, qv, float(r), relop))
    for i in range(n):
        if name == 'box3':
            if i % 3 == 0:
                quad(i, 1.0, 0.0, -1.0, '<=')
            elif i % 3 == 1:
                quad(i, 1.0, 0.0, -0.49, '<=')
            else:
                quad(i, 1.0, -0.5, -0.5, '<=')
        elif name == 'ann2':
            if i % 2 == 0:
                quad(i, 1.0, 0.0, -1.0, '<=')
                quad(i, -1.0, 0.0, 0.25, '<=')
            else:
                quad(i, 1.0, 0.0, -1.0, '==')
        elif name == 'lin2':
            lo, hi = ((-0.75, 1.25), (-1.5, 0.5))[i % 2]
            quad(i, 0.0, 1.0, -hi, '<=')
            quad(i, 0.0, -1.0, lo, '<=')
        elif name == 'cut2':
            quad(i, 1.0, 0.0, -1.0, '==' if i % 2 == 0 else '<=')
        elif name in ('box4', 'cut4'):
            c = i % 4
            if c == 3:
                quad(i, 1.0, 0.0, -1.0, '<=')
                quad(i, -1.0, 0.0, 0.25, '<=')
            elif name == 'box4':
                quad(i, 1.0, -0.5 if c == 2 else 0.0, (-1.0, -0.49, -0.5)[c], '<=')
            else:
                quad(i, 1.0, 0.0, (-1.0, -1.0, -0.49)[c], '==' if c == 0 else '<=')
        else:
            raise KeyError(name)
    return funcs


def maxcut(n, p=0.5, seed=1, weighted=False):
    """maximize 0.25 (sum(W) - x^T W x)  s.t. x_i^2 == 1   (minimise form returned).
    weighted=True draws edge weights from U(0.5, 1.5): no exact ties between cuts."""
    rs = np.random.RandomState(seed)
    U = np.triu((rs.uniform(size=(n, n)) < p).astype(float), 1)
    if weighted:
        U = U * np.triu(rs.uniform(0.5, 1.5, size=(n, n)), 1)
    W = U + U.T
    P0 = 0.25 * W
    r0 = -0.25 * float(W.sum())
    funcs = [(P0, np.zeros(n), r0, None)]
    for i in range(n):
        P = sp.csr_matrix(([1.0], ([i], [i])), shape=(n, n))
        funcs.append((P, np.zeros(n), -1.0, '=='))
    return funcs, True, dict(W=W)


def beamforming(nant, m_h, l, tau=20., eta=2., seed=1):
    """minimize ||x||^2 s.t. |h_i^H x|^2 >= tau, |g_i^H x|^2 <= eta, real expansion (n = 2 nant)."""
    rs = np.random.RandomState(seed)
    HR = rs.randn(m_h, nant)
    HI = rs.randn(m_h, nant)
    A = np.hstack((HR, HI))
    B = np.hstack((-HI, HR))
    GR = rs.randn(l, nant)
    GI = rs.randn(l, nant)
    Cm = np.hstack((GR, GI))
    D = np.hstack((-GI, GR))
    n = 2 * nant
    funcs = [(np.eye(n), np.zeros(n), 0.0, None)]
    for i in range(m_h):
        P = -(np.outer(A[i], A[i]) + np.outer(B[i], B[i]))
        funcs.append((P, np.zeros(n), tau, '<='))
    for i in range(l):
        P = np.outer(Cm[i], Cm[i]) + np.outer(D[i], D[i])
        funcs.append((P, np.zeros(n), -eta, '<='))
    return funcs, False, dict(A=A, B=B, C=Cm, D=D)


def dense_indefinite(n, m, seed=7, easy=True):
    """Random indefinite dense QCQP: P_k = (G+G^T)/2, G = randn/sqrt(n); last constraint is the
    ball ||x||^2 <= n.  easy=True scales r_k with n so that feasibility is reachable."""
    rs = np.random.RandomState(seed)

    def sym():
        G = rs.randn(n, n) / np.sqrt(n)
        return (G + G.T) / 2.

    funcs = [(sym(), rs.randn(n), 0.0, None)]
    for k in range(m - 1):
        r = -1. - abs(rs.randn())
        if easy:
            r *= n / 8.
        funcs.append((sym(), rs.randn(n), r, '<='))
    funcs.append((np.eye(n), np.zeros(n), -float(n), '<='))
    return funcs, False, {}


def circle_packing(N, B=10., minimize_form=False):
    """maximize r  s.t.  r <= X <= B - r, r >= 0, (2r)^2 <= ||X[:, i] - X[:, j]||^2 for i < j
    (examples/circle_packing.py:6-17: N circles of radius r in the box [0, B]^2).  Two cvxpy variables in the reference --
    X (2, N) and the scalar r; get_qcqp_form (utilities.py:318-347) stacks them in the order prob.variables() gives them,
    each flattened COLUMN-major (utilities.py:298-316): here x = [X[0,0], X[1,0], X[0,1], ..., X[1,N-1], r], n = 2 N + 1,
    var_sizes [(2, N), (1, 1)].  Constraints in the order of the example's list: 2 N of r - X[d, i] <= 0 (column-major),
    2 N of X[d, i] + r - B <= 0, -r <= 0, then the N (N - 1) / 2 separation constraints 4 r^2 - ||X_i - X_j||^2 <= 0 (sparse,
    indefinite, five coordinates each).  Returns (funcs, maximize, info): funcs as stated (objective = r, to be maximised;
    minimize_form=True: already negated, what QCQPForm holds), info['var_sizes']."""
    import scipy.sparse as sp
    n = 2 * N + 1
    ir = 2 * N
    q0 = np.zeros(n)
    q0[ir] = -1.0 if minimize_form else 1.0
    funcs = [(sp.csr_matrix((n, n)), q0, 0.0, None)]
    Z = sp.csr_matrix((n, n))
    for j in range(2 * N):                       # X >= r
        q = np.zeros(n)
        q[ir], q[j] = 1.0, -1.0
        funcs.append((Z, q, 0.0, '<='))
    for j in range(2 * N):                       # X <= B - r
        q = np.zeros(n)
        q[ir], q[j] = 1.0, 1.0
        funcs.append((Z, q, -float(B), '<='))
    q = np.zeros(n)
    q[ir] = -1.0
    funcs.append((Z, q, 0.0, '<='))              # r >= 0
    for i in range(N):
        for j in range(i + 1, N):
            rows, cols, vals = [ir], [ir], [4.0]
            for d in range(2):
                a, b = 2 * i + d, 2 * j + d
                rows += [a, b, a, b]
                cols += [a, b, b, a]
                vals += [-1.0, -1.0, 1.0, 1.0]
            funcs.append((sp.csr_matrix((vals, (rows, cols)), shape=(n, n)), np.zeros(n), 0.0, '<='))
    return funcs, (not minimize_form), dict(var_sizes=[(2, N), (1, 1)], B=float(B))


class GeneratedForm(object):
    """A QCQP whose dense functions are synthesised ON THE DEVICE from a seed
    (qcqpmi_set_quad_generated; BASELINE.json configs[4] at full size is 137.6 GB of matrices).
    specs[0] is the objective; every entry: seed, scale, qscale, diag_add, r, relop."""

    def __init__(self, n, specs):
        self.n, self.m, self.specs = int(n), len(specs) - 1, list(specs)


def dense_indefinite_generated(n, m, seed=7, easy=True):
    """The dense_indefinite family with device-side generation: P_k ~ (G+G^T)/2, G = randn/sqrt(n)
    (same law, symmetric by construction), q_k = randn, r_k = -(1+|z_k|) [* n/8], last constraint the
    ball ||x||^2 <= n."""
    rs = np.random.RandomState(seed)
    sc = 1.0 / np.sqrt(n)
    specs = [dict(seed=seed, scale=sc, qscale=1.0, diag_add=0.0, r=0.0, relop=None)]
    for k in range(m - 1):
        r = -1. - abs(rs.randn())
        if easy:
            r *= n / 8.
        specs.append(dict(seed=seed, scale=sc, qscale=1.0, diag_add=0.0, r=r, relop='<='))
    specs.append(dict(seed=seed, scale=0.0, qscale=0.0, diag_add=1.0, r=-float(n), relop='<='))
    return GeneratedForm(n, specs)


def materialise_generated(form, keyed_normal):
    """The same functions as NumPy arrays (small n only): keyed_normal(seed, stream, elem) is the
    oracle's orc_keyed_normal.  Returns the usual [(P, q, r, relop), ...] list."""
    n = form.n
    funcs = []
    for k, g in enumerate(form.specs):
        P = np.zeros((n, n))
        q = np.zeros(n)
        for i in range(n):
            for j in range(i, n):
                v = g['scale'] * keyed_normal(g['seed'], (1 << 48) + k, i * n + j) if g['scale'] != 0.0 else 0.0
                if i == j:
                    P[i, i] = v + g['diag_add']
                else:
                    P[i, j] = P[j, i] = v * 0.70710678118654752440
            if g['qscale'] != 0.0:
                q[i] = g['qscale'] * keyed_normal(g['seed'], (2 << 48) + k, i)
        funcs.append((P, q, g['r'], g['relop']))
    return funcs
