"""What tests/test_eval_reference_cpu.py and tests/test_gpu_eval_domain.py share: a plain high-precision reference of the evaluation
and product operators (Engine.eval, eval_parts, weighted_matrix, weighted_product, sdr_sample), the DERIVED rounding bounds the device
results are held to, the seeded inputs, a restatement of dense_zsplit and the case tables.  A plain module, not a conftest: the test
files import what they use.

REFERENCE.  f_k(x) = x' P_k x + q_k' x + r_k on the symmetrised matrices (P + P') / 2 -- formed exactly as QCQPForm.from_arrays and
Engine._set_quad form them, so the reference and the device hold the same bits --, the violations ('<=': max(f, 0), '==': |f|) and
their maximum over k >= 1.  Two tiers: every column in float64 NumPy, and a sample of columns in np.longdouble (64-bit mantissa;
exact fractions.Fraction arithmetic on at least 4 columns where a machine has no such type).

BOUND.  With u = 2^-53 and A_k(x) = |x|' |P_k| |x| + |q_k|' |x| + |r_k|, ANY fp64 evaluation made of an n16-term dot product per row,
an n16-term dot product of those rows with x and a handful of plane, linear and constant additions satisfies
|fl(f) - f| <= K u A_k(x) with K = 2 n16 + 32, whatever the order of the additions and with or without FMA: every product x_i P_ij x_j
passes through at most n16 additions inside its row, one multiplication by x_i, at most n16 additions across the rows and at most 32
more (16 lane-group partials, <= 8 partial planes, the linear part, r_k, the two shuffles), each of which multiplies it by one
(1 + delta), |delta| <= u; the linear terms pass through fewer.  (1 + u)^K - 1 <= 1.0001 K u for K < 1e4, which the factor 2 of the
float64 tier and the 64-bit reference absorb.  The bound is a statement about the operation, not about this code: nothing here is
measured.
  K_dense(n)      = 2 n16 + 32       MFMA evaluations (dense_products_kernel<1>, <2>, eval_kernel's per-tile loop)
  K_coo(nnz, n)   = nnz + n + 4      the COO loop of eval_kernel: nnz products added one by one, n linear terms, s + l + r
  K_SEP           = 4                a separable constraint (p x + q) x + r: four roundings at most
  device against the longdouble tier: <= K u A;  against the float64 tier: <= 2 K u A (both sides are fp64 evaluations)
  max violation: max over k of the per-function bounds (max, |.| and max(., 0) are 1-Lipschitz)
No path has needed a term-count correction so far (a path that exceeds the bound while correct gets its extra additions named
HERE and added to K; the bound is never scaled).

The other operators, by the same argument:
  eval_parts       quad[k] against x'P_k x + r_k: K_dense u (|x|'|P_k||x| + |r_k|);  lin[k] against q_k'x: (n16 + 2) u |q_k|'|x|
  weighted_matrix  sum_k w_k P_k: (m + 3) u sum_k |w_k| |P_k|  (m + 1 products, m + 1 additions in two chains and their sum)
  weighted_product (sum_k w_k P_k) X: (n16 + m + 5) u (sum_k |w_k| |P_k|) |X|  (the sum above, then an n16-term dot product and + 0)
  sdr_sample       mu + F xi: (n16 + 2) u (|mu| + |F| |xi|)
"""
import fractions

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
LD = np.longdouble
LD_OK = np.finfo(LD).nmant >= 63          # x87 extended or better; else the sample tier is exact rational arithmetic
K_SEP = 4


def n16_of(n):
    return (int(n) + 15) // 16 * 16


def K_dense(n):
    return 2 * n16_of(n) + 32


def K_coo(nnz, n):
    return int(nnz) + int(n) + 4


# ------------------------------------------------------------------------------------------- dense_zsplit, restated
def dense_zsplit_expected(m1, ntiles, NB):
    """csrc/capi_dense.hip:dense_zsplit without its environment override: grid.z of dense_products_kernel<0> / <1>."""
    wg = ((m1 + 7) // 8) * ((ntiles + 7) // 8)
    zs = 1
    if wg < 512:
        best = 1e30
        for z in range(1, 8):
            cost = float((wg * z + 511) // 512) / z + 0.02 * z
            if cost < best - 1e-12:
                best, zs = cost, z
    return max(1, min(zs, 7, NB))


def natural_zs(n, m, R):
    return dense_zsplit_expected(m + 1, (R + 15) // 16, n16_of(n) // 16)


# ------------------------------------------------------------------------------------------------------ case tables
# 3a: coupled constraints (n, m, R) -> what the shape exercises
COUPLED_CASES = [
    (65, 1, 1),        # one tile, narrow arrangement
    (80, 7, 17),       # m + 1 = 8: exactly one function group
    (80, 8, 64),       # second group holds one function; 4 tiles: the narrow boundary
    (96, 12, 65),      # NB = 6 so zs = 6; 5 tiles: wide arrangement, one valid tile in the second wave column
    (100, 7, 112),     # ragged n, zs = 7, 7 tiles
    (112, 17, 129),    # full tile group plus a narrow group of 1
    (127, 3, 208),     # full group plus a wide partial group
    (129, 63, 33),     # m + 1 = 64 = m1p
    (70, 64, 48),      # m1p = 128
]
NATURAL_ZS_CASES = [((80, 130, 4096), 1), ((80, 63, 4096), 2), ((96, 64, 2048), 3), ((96, 63, 2048), 4),
                    ((80, 8, 64), 5), ((96, 12, 65), 6), ((100, 7, 112), 7)]
FORCED_ZS_CASE = (112, 9, 40)
DEBUG_DENSE_CASES = [(5, 2, 3), (16, 3, 16), (17, 4, 17), (33, 5, 5), (64, 6, 20)]      # the dense path at n <= 64 (debug switch)
# 3b: separable constraints (n, R): per-tile MFMA loop against the planes path (NB >= 8 and ntiles >= 8)
SEP_CASES = [(5, 3), (16, 16), (17, 1), (64, 100), (112, 200), (113, 112), (113, 113), (128, 128), (130, 200), (257, 129),
             (272, 100), (320, 96)]
SEP_FAMILIES = ('bls', 'cut', 'ann2', 'boxz')
# 3c: the COO loop (non-separable, n <= 64, no debug switch)
COO_CASES = [(5, 2), (16, 3), (17, 4), (64, 20)]
COO_RS = (1, 16, 37)
PARTS_CASES = [(65, 1, 1), (80, 8, 64), (100, 7, 112), (112, 17, 129), (70, 64, 48)]      # (80, 8, 64): zs = 5, (100, 7, 112): zs = 7
WMAT_NS, WMAT_DEBUG_NS = (65, 100, 128), (5, 17)
WPROD_RS = (1, 47, 64, 65, 129)
WPROD_COUPLED_NS, WPROD_SEP_NS = (65, 100, 130), (40, 112, 130)
SAMPLE_CASES = [(112, 112), (112, 113), (113, 112), (113, 113), (130, 47)]
SELECT_RS = (1, 15, 1023, 1024, 1025, 2500)


def sep_takes_planes(n, R):
    """launch_eval's switch (csrc/capi.hip): the LDS-tiled GEMM with partial planes instead of eval_kernel's per-tile loop."""
    return n16_of(n) // 16 >= 8 and (R + 15) // 16 >= 8


# ----------------------------------------------------------------------------------------------------------- inputs
def population(n, R, seed):
    """(n, R) points; column r scaled by 10^uniform(-3, 3)."""
    rs = np.random.RandomState(seed)
    return rs.randn(n, R) * 10.0 ** rs.uniform(-3.0, 3.0, size=R)


def coupled_problem(n, m, seed, csr=True):
    """problems.dense_indefinite(n, m) with constraint k scaled by 10^uniform(-2, 2), q and r nonzero everywhere, every third
    constraint an '==', a skew-symmetric part added to every even function (x'Px does not see it; the symmetrisation at upload
    must remove it) and function max(1, m // 2) handed over as CSR."""
    from qcqp_amd import problems
    funcs = problems.dense_indefinite(n, m, seed=seed)[0]
    rs = np.random.RandomState(10007 + seed)
    out = []
    for k, (P, q, r, rel) in enumerate(funcs):
        s = 10.0 ** rs.uniform(-2.0, 2.0) if k >= 1 else 1.0
        P = np.asarray(P, dtype=np.float64) * s
        q = (q if np.any(q != 0.0) else rs.randn(n)) * s
        r = (r if r != 0.0 else 1.0 + abs(rs.randn())) * s
        G = rs.randn(n, n) * (0.25 * s / np.sqrt(n))
        if k % 2 == 0:
            P = P + (G - G.T)
        if k >= 1 and k % 3 == 0:
            rel = '=='
        if csr and k == max(1, m // 2):
            P = sp.csr_matrix(P)
        out.append((P, q, float(r), rel))
    return out


def sep_family(name, n, seed=1):
    """The separable families of section 3b."""
    from qcqp_amd import problems
    if name == 'bls':       # dense P0, x_i^2 == 1
        return problems.boolean_least_squares(n, n + n // 2 + 1, seed=seed)[0]
    if name == 'cut':       # weighted MAXCUT, P0 handed over as CSR
        funcs = problems.maxcut(n, seed=seed, weighted=True)[0]
        P0, q0, r0, rel = funcs[0]
        return [(sp.csr_matrix(P0), q0, r0, rel)] + funcs[1:]
    if name == 'ann2':      # two constraints on the even coordinates, both relops
        return problems.multi_class('ann2', n, seed=seed)
    if name == 'boxz':      # indefinite objective with zeros on the diagonal, linear terms in the constraints
        return problems.box_qp(n, seed=seed, zero_every=3)[0]
    raise KeyError(name)


def symmetrised(funcs):
    """[(P, q, r, relop)] with P = (P + P') / 2 formed as QCQPForm.from_arrays forms it (dense stays dense, sparse stays CSR)."""
    out = []
    for P, q, r, rel in funcs:
        if sp.issparse(P):
            P = sp.csr_matrix((P + P.T) / 2.)
        else:
            P = np.asarray(P, dtype=np.float64)
            P = (P + P.T) / 2.
        out.append((P, np.asarray(q, dtype=np.float64).ravel(), float(r), rel))
    return out


def dense_of(P):
    return np.asarray(P.todense()) if sp.issparse(P) else np.asarray(P)


def nnz_of(P):
    return int(np.count_nonzero(P.data)) if sp.issparse(P) else int(np.count_nonzero(P))


def sample_columns(R, seed=0, count=32):
    """At least `count` columns (all of them when R is smaller): 0, 15, 16, R - 1, every tile-group edge 128 j - 1 and 128 j, the
    rest from a seeded RNG."""
    if R <= count:
        return np.arange(R)
    cols = {0, 15, 16, R - 1}
    for j in range(1, (R + 127) // 128 + 1):
        cols.update(c for c in (128 * j - 1, 128 * j) if c < R)
    rs = np.random.RandomState(977 + seed)
    while len(cols) < count:
        cols.add(int(rs.randint(R)))
    return np.array(sorted(cols))


# -------------------------------------------------------------------------------------------------------- reference
def quad_values(P, q, r, X, dtype=np.float64):
    """x'Px + q'x + r for every column of X in `dtype` arithmetic (float64: BLAS / SciPy products; longdouble: NumPy's plain loops)."""
    Xd = X.astype(dtype)
    if sp.issparse(P):
        Pc = P.tocoo()
        if dtype == np.float64:
            quad = np.asarray((Xd * (P @ Xd)).sum(axis=0)).ravel()
        else:
            quad = (Pc.data.astype(dtype)[:, None] * Xd[Pc.row] * Xd[Pc.col]).sum(axis=0) if Pc.nnz else np.zeros(X.shape[1], dtype=dtype)
    else:
        quad = (Xd * (P.astype(dtype) @ Xd)).sum(axis=0)
    return quad + q.astype(dtype) @ Xd + dtype(r)


def magnitude(P, q, r, X):
    """A_k(x) = |x|'|P||x| + |q|'|x| + |r| per column."""
    Xa = np.abs(X)
    return quad_values(abs(P), np.abs(q), abs(r), Xa)


def quad_fraction(P, q, r, x):
    """The same value in exact rational arithmetic for ONE point."""
    Fr = fractions.Fraction
    xs = [Fr(float(v)) for v in x]
    Pc = sp.coo_matrix(P)
    s = Fr(float(r))
    for i, j, v in zip(Pc.row, Pc.col, Pc.data):
        s += Fr(float(v)) * xs[int(i)] * xs[int(j)]
    for j, v in enumerate(q):
        s += Fr(float(v)) * xs[j]
    return s


def violations(F, relops):
    """(m, R) violations of rows 1.. of F; relops[k] for k = 0..m (relops[0] is None)."""
    V = np.empty_like(F[1:])
    for k in range(1, F.shape[0]):
        V[k - 1] = np.abs(F[k]) if relops[k] == '==' else np.where(F[k] > 0, F[k], np.zeros_like(F[k]))      # +0.0, never -0.0
    return V


def max_violation(F, relops):
    return violations(F, relops).max(axis=0)


class Reference(object):
    """Both tiers and the magnitudes of one (problem, population): F64, A (m + 1, R); cols, FLD (m + 1, len(cols)).
    K: one term count per function."""

    def __init__(self, funcs, X, K, seed=0, count=32):
        self.funcs = symmetrised(funcs)
        self.X = np.asarray(X, dtype=np.float64)
        self.relops = [f[3] for f in self.funcs]
        m1, R = len(self.funcs), self.X.shape[1]
        self.K = np.broadcast_to(np.asarray(K, dtype=np.float64), (m1,)).reshape(m1, 1)
        self.F64 = np.empty((m1, R))
        self.A = np.empty((m1, R))
        self.cols = sample_columns(R, seed, count) if LD_OK else sample_columns(R, seed, count)[:4]
        Xs = self.X[:, self.cols]
        self.FLD = np.empty((m1, self.cols.size), dtype=LD)
        for k, (P, q, r, rel) in enumerate(self.funcs):
            self.F64[k] = quad_values(P, q, r, self.X)
            self.A[k] = magnitude(P, q, r, self.X)
            if LD_OK:
                self.FLD[k] = quad_values(P, q, r, Xs, LD)
            else:
                self.FLD[k] = [LD(float(quad_fraction(P, q, r, Xs[:, c]))) for c in range(self.cols.size)]
        self.bound = self.K * U * self.A                       # per function and column
        self.mv64 = max_violation(self.F64, self.relops) if m1 > 1 else None
        self.mvLD = max_violation(self.FLD, self.relops) if m1 > 1 else None
        self.mv_bound = self.bound[1:].max(axis=0) if m1 > 1 else None

    def ratios(self, F, maxviol=None):
        """Worst error / bound of device values F (m + 1, R) [and maxviol (R,)] against the two tiers: (longdouble tier,
        float64 tier); <= 1 passes.  0 / 0 counts as 0, x / 0 as inf."""
        F = np.asarray(F, dtype=np.float64)

        def worst(err, bound):
            err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                q = np.where(err == 0.0, 0.0, err / bound)
            return float(np.max(np.where(np.isnan(q), np.inf, q))) if q.size else 0.0
        rl = worst(np.abs(F[:, self.cols].astype(LD) - self.FLD), self.bound[:, self.cols])
        rd = worst(np.abs(F - self.F64), 2.0 * self.bound)
        if maxviol is not None and self.mv64 is not None:
            mv = np.asarray(maxviol, dtype=np.float64)
            rl = max(rl, worst(np.abs(mv[self.cols].astype(LD) - self.mvLD), self.mv_bound[self.cols]))
            rd = max(rd, worst(np.abs(mv - self.mv64), 2.0 * self.mv_bound))
        return rl, rd

    def accepts(self, F, maxviol=None):
        rl, rd = self.ratios(F, maxviol)
        return rl <= 1.0 and rd <= 1.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def device_max_violation(F, relops):
    """The maximum violation of the device's OWN function values, as dense_viol_kernel and eval_kernel form it: exact operations
    only (|f|, f > 0 ? f : 0, max), so the device's maxviol must equal it bit for bit."""
    return max_violation(np.asarray(F, dtype=np.float64), relops)


def eval_K(funcs, path):
    """Term counts per function for the path an evaluation takes: 'dense' (MFMA for every function), 'sep' (objective on the
    matrix cores, constraints element-wise) or 'coo' (objective on the matrix cores, constraints by the COO loop)."""
    fs = symmetrised(funcs)
    n = fs[0][1].size
    if path == 'dense':
        return [K_dense(n)] * len(fs)
    if path == 'sep':
        return [K_dense(n)] + [K_SEP] * (len(fs) - 1)
    if path == 'coo':
        return [K_dense(n)] + [K_coo(nnz_of(f[0]), n) for f in fs[1:]]
    raise KeyError(path)


# ------------------------------------------------------------------------------------ the other operators, longdouble
def weighted_sum_ld(funcs, w):
    """(sum_k w_k P_k, sum_k |w_k| |P_k|) of the symmetrised matrices in longdouble / float64."""
    fs = symmetrised(funcs)
    n = fs[0][1].size
    S, M = np.zeros((n, n), dtype=LD), np.zeros((n, n))
    for wk, f in zip(w, fs):
        if wk != 0.0:
            Pd = dense_of(f[0])
            S += LD(wk) * Pd.astype(LD)
            M += abs(wk) * np.abs(Pd)
    return S, M


def wmat_bound(m, M):
    return (m + 3) * U * M


def wprod_reference(funcs, w, X):
    """((sum_k w_k P_k) X in longdouble, its bound (n16 + m + 5) u (sum |w_k||P_k|) |X|)."""
    S, M = weighted_sum_ld(funcs, w)
    n, m = X.shape[0], len(funcs) - 1
    return S @ X.astype(LD), (n16_of(n) + m + 5) * U * (M @ np.abs(X))


def sample_reference(mu, Fm, Xi):
    """(mu + F xi in longdouble, its bound (n16 + 2) u (|mu| + |F||xi|))."""
    n = mu.size
    ref = mu.astype(LD)[:, None] + Fm.astype(LD) @ Xi.astype(LD)
    return ref, (n16_of(n) + 2) * U * (np.abs(mu)[:, None] + np.abs(Fm) @ np.abs(Xi))


def worst_ratio(dev, ref, bound):
    err = np.abs(np.asarray(dev).astype(LD) - ref).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(np.where(np.isnan(q), np.inf, q))) if q.size else 0.0


# --------------------------------------------------------------------- host-made WRONG evaluations (the checker must refuse them)
def blocked_eval(funcs, X, zs=1, drop_last_block=False, drop_last_plane=False, r_per_plane=False, pad_ones=False, reverse=True):
    """A host twin of dense_products_kernel<1>'s ORDER in float64: row blocks of 16 split into zs slices (planes), the rows of a
    block and the blocks of a slice added in REVERSED order, planes added last, then the linear part -- and, on request, one of
    the faults a kernel of this shape can have.  Returns F (m + 1, R)."""
    fs = symmetrised(funcs)
    n, R = X.shape
    n16 = n16_of(n)
    NB = n16 // 16
    zs = max(1, min(zs, NB))
    Xp = np.zeros((n16, R))
    Xp[:n] = X
    if pad_ones:
        Xp[n:] = 1.0
    F = np.empty((len(fs), R))
    for k, (P, q, r, rel) in enumerate(fs):
        Pp = np.ones((n16, n16)) if pad_ones else np.zeros((n16, n16))
        Pp[:n, :n] = dense_of(P)
        planes = []
        for z in range(zs):
            b_lo, b_hi = z * NB // zs, (z + 1) * NB // zs
            acc = np.zeros(R)
            blocks = range(b_lo, b_hi)
            for b in (reversed(blocks) if reverse else blocks):
                if drop_last_block and b == NB - 1:
                    continue
                rows = range(16 * b, 16 * b + 16)
                for i in (reversed(rows) if reverse else rows):
                    acc = acc + Xp[i] * (Pp[i] @ Xp)
            if z == 0 or r_per_plane:
                acc = acc + r
            planes.append(acc)
        if drop_last_plane:
            planes = planes[:-1]
        f = planes[0]
        for p in planes[1:]:
            f = f + p
        F[k] = f + q @ X
    return F
