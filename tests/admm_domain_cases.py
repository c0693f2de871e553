"""What tests/test_admm_domain_cpu.py and tests/test_gpu_admm_domain.py share: a plain reference of onecons_qcqp IN A BASIS
(utilities.py:149-196 as csrc/admm.h evaluates it), the DERIVED rounding bound the device is held to, a restatement of the launch
conditions of csrc/capi_admm.hip (admm_launch_secular, gemm_pk, gemm_zsplit), the seeded generators and the case tables.  A plain
module, not a conftest, and it imports no GPU code.

REFERENCE (onecons_basis).  Given the eigenvalues lam, qhat = B q, r, the relop, the bracket (slo, ehi) and vhat = B z of ONE
(constraint, point) pair it replays the reference's search: the early return of a feasible '<=' point, the doubling of an open
bracket end, the bisection to 1e-6.  The bracket s, e and the midpoints are carried in float64 with the reference's own expressions
((s + e) / 2., s *= 2.), so the sequence of trial multipliers is reproducible bit for bit by anything that takes the same DECISIONS
(the sign of phi at every trial).  What differs between the tiers is the arithmetic of phi and of the final xhat:
  'ld'      np.longdouble throughout (64-bit mantissa): the yardstick;
  'seq'     float64, IEEE division, the sums added one by one in index order;
  'kernel'  float64, IEEE division, the sums in the order of admm_secular_kernel<EPL, NW>: element j of lane l in slot e is
            j = l + 64 NW e, every lane adds its slots in order, the 64 lanes of a wave are summed by a balanced tree of neighbours
            (the DPP row_shr 1, 2, 4, 8, row_bcast 15, 31 sequence), the four waves of NW = 4 one after the other;
            for a reduced basis of <= 8 rows the order of admm_small_solve: p += lam x^2 + qhat x, element by element.
Every tier returns xhat, the final multiplier, the decision string and the smallest |phi(trial)| / scale it met, where
scale = sum |lam| xhat^2 + sum |qhat xhat| + |r| at that trial.  Two evaluations of phi whose error is far below that margin take the
same decisions; then they hold the same multiplier nu, bit for bit, and differ only by the rounding of xhat(nu):

BOUND (xhat_bound), u = 2^-53, for one element with num = -(nu qhat - 2 vhat), den = 2 (1 + nu lam), xhat = num / den:
  num   fl(nu qhat) = nu qhat (1 + d1); 2 vhat is exact; the subtraction rounds once (the negation is exact):
        |fl(num) - num| <= u (1 + u) |nu qhat| + u |num|                                            =: e_num
        (an error e_v of vhat itself -- it is the result of a product B z on the device -- adds 2 e_v)
  den   fl(nu lam) = nu lam (1 + d1), fl(1 + .) rounds once, the factor 2 is exact:
        |fl(den) - den| / |den| <= u (1 + u) (|nu lam| / |1 + nu lam| + 1) <= u (1 + u) (C + 1)     =: r_den
        with the CANCELLATION FACTOR C = (1 + |nu lam|) / |1 + nu lam| (lam = 0: den = 2 exactly, r_den = 0)
  division  admm_div: r0 = v_rcp_f64(den) with relative error e0 (any e0 <= 2^-14 will do), two Newton steps
        r <- fma(fma(-den, r, 1), r, r): the residual t = 1 - den r is one rounding of a number of size e (error u e), the exact
        update squares the error, the last fma rounds once: e1 <= e0^2 + 2 u, e2 <= e1^2 + u (1 + 2^-20) <= 1.01 u; num * r rounds
        once more: relative error of the quotient <= 2.25 u =: r_div  (IEEE division of the float64 tiers: u)
  xhat  |fl(xhat) - xhat| <= ((e_num + 2 e_v) / |den|) (1 + r_den + r_div) / (1 - r_den) + |xhat| (r_den / (1 - r_den) + r_div)
        (an element slot whose eigenvalues are zero in every lane multiplies by 0.5 instead: exact, covered)
The yardstick's own error is the same expression with u = 2^-64 and is added.  lam = 0 and qhat = 0 give xhat = vhat exactly.

OUTPUT (ACase.reference, eig_reference), gamma_k = k u / (1 - k u), k counting the NONZERO terms of a contraction (products with an exact zero and
additions of an exact zero are exact, whatever the order of the additions and with or without FMA; the padding is zeros):
  reduced basis (qcqpmi_admm_set_basis)   x = z + B' (xhat - B z):
        e_v = gamma_kB |B| |z|                        (kB nonzeros per row of B)
        d = fl(xhat - zq):  e_d <= e_xhat + e_v + u (|d| + e_xhat + e_v)
        |x_dev - x| <= |B|' e_d + gamma_kT |B|' (|d| + e_d) + u (|x| + all of the former)      (kT nonzeros per column of B)
        a signed permutation has kB = kT = 1 and s = +-1: B z and B' d are exact, what is left is the rounding of xhat, of the
        subtraction and of the last addition -- the secular kernels in isolation.
  full eigenbasis (qcqpmi_admm_set_eig)   x = Q xhat, vhat = Q' z:
        e_v = gamma_n |Q|' |z|;    |x_dev - x| <= |Q| e_xhat + gamma_n |Q| (|xhat| + e_xhat)
  the two products alone (lam = 0, q = 0, r < 0: always feasible, xhat = vhat bit for bit) with ANY matrix Q:
        |x_dev - Q Q' z| <= (2 gamma_n + gamma_n^2) |Q| (|Q|' |z|)                               (gemm_bound)
Against another float64 evaluation (the oracle, NumPy) both sides carry the bound: 2 x.  Nothing here is fitted to the device.
"""
import fractions

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
LD = np.longdouble
ULD = float(np.finfo(LD).eps) / 2.0        # 2^-64 with the x87 type (a machine whose longdouble is float64 gets u: the bound doubles)
R_DIV = 2.25
MARGIN_MIN = 1e3 * U                       # smallest |phi(trial)| / scale a case may meet (equal decisions in every tier)
CANCEL_MAX = 1e6                           # largest cancellation factor at the final multiplier
SEC_TOL = 1e-6


def n16_of(n):
    return (int(n) + 15) // 16 * 16


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------- launch conditions, restated
SMALL_ROWS = (1, 2, 4, 8)
WAVE_LIMITS = ((128, 2, 1), (256, 4, 1), (512, 8, 1), (1024, 16, 1), (2048, 32, 1), (4096, 64, 1), (8192, 32, 4), (16384, 64, 4))
ALL_SECULAR = ['small<%d>' % r for r in SMALL_ROWS] + ['wave<%d,%d>' % (e, w) for _, e, w in WAVE_LIMITS]


def secular_instantiation(rows, lowrank):
    """admm_launch_secular (csrc/capi_admm.hip): which kernel solves the secular equations; None = refused."""
    if lowrank and rows <= 8:
        return 'small<%d>' % rows if rows in SMALL_ROWS else None
    for lim, epl, nw in WAVE_LIMITS:
        if rows <= lim:
            return 'wave<%d,%d>' % (epl, nw)
    return None                            # more than 16384 rows: refused by qcqpmi_admm_run


def wave_geometry(rows, lowrank):
    """(EPL, stride between the element slots of a lane) of the wave kernel, or None for the small kernels."""
    name = secular_instantiation(rows, lowrank)
    if name is None or name.startswith('small'):
        return None
    epl, nw = [int(t) for t in name[5:-1].split(',')]
    return epl, 64 * nw


def gemm_kernel(MB, KB, ntiles, zs=1):
    """gemm_pk: 128 x 128 outputs per workgroup once there are 256 such workgroups, else 64 x 64."""
    wg_big = ((MB + 7) // 8) * ((ntiles + 7) // 8) * zs
    return 'gemm_pk_small_kernel' if wg_big < 256 else 'gemm_pk_kernel'


def gemm_zsplit(MB, ntiles, KB):
    wg = ((MB + 7) // 8) * ((ntiles + 7) // 8)
    zs = (512 + wg - 1) // wg
    return max(min(zs, 16, KB // 8), 1)


def geometry(n, m, rows, lowrank, R, unit=False):
    """Everything the multi-launch path chooses for one shape: the two products (ZQ = W' Z: MB = hat row blocks, KB = n blocks;
    S = W D: the other way round), their planes in qcqpmi_admm_run (the unit operator uses one plane), the secular kernel and the
    violation reduction of admm_secular_small_kernel."""
    KBn, MBh, ntiles = n16_of(n) // 16, n16_of(m * rows) // 16, n16_of(R) // 16
    small = bool(lowrank) and rows <= 8
    zs1 = 1 if unit else (gemm_zsplit(MBh, ntiles, KBn) if small else 1)
    zs2 = 1 if unit else gemm_zsplit(KBn, ntiles, MBh)
    return dict(KBn=KBn, MBh=MBh, ntiles=ntiles, secular=secular_instantiation(rows, lowrank),
                gemm1=gemm_kernel(MBh, KBn, ntiles, 1), gemm2=gemm_kernel(KBn, MBh, ntiles, 1),
                run_zs1=zs1, run_zs2=zs2, run_gemm1=gemm_kernel(MBh, KBn, ntiles, zs1), run_gemm2=gemm_kernel(KBn, MBh, ntiles, zs2),
                viol_reduction=('lds' if m % 16 == 0 else 'atomic') if small else 'wave')


def smallest_first_product_big(ns=range(17, 132), ms=range(1, 65)):
    """The cheapest (n, m, R), n not a multiple of 16, full basis, at which ZQ = W' Z takes gemm_pk_kernel and S = W D does not;
    cost = the multiplications of one product, m n16^2 Rpad."""
    best = None
    for n in ns:
        if n % 16 == 0:
            continue
        KBn = n16_of(n) // 16
        for m in ms:
            MBh = n16_of(m * n) // 16
            need = -(-256 // ((MBh + 7) // 8))             # ceil(ntiles / 8) must reach this
            ntiles = 8 * (need - 1) + 1
            if ((KBn + 7) // 8) * need >= 256:
                continue
            cost = m * n16_of(n) ** 2 * ntiles * 16
            if best is None or cost < best[0]:
                best = (cost, n, m, 16 * ntiles - 3)       # three columns short of a full last tile
    return best[1:]


# ----------------------------------------------------------------------------------------------- the reference
def _tree64(v):
    """Sum of 64 lanes by a balanced tree of neighbours (wave_sum of csrc/admm.h up to the commutativity of an addition)."""
    v = np.asarray(v)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _sum_seq(x):
    return float(np.add.accumulate(np.asarray(x, dtype=np.float64))[-1]) if len(x) else 0.0


def _sum_kernel(x, stride):
    """Lane-strided partial sums, a tree per wave, the waves in order."""
    x = np.asarray(x, dtype=np.float64)
    epl = -(-len(x) // stride)
    pad = np.zeros(epl * stride)
    pad[:len(x)] = x
    lanes = np.zeros(stride)
    for e in range(epl):
        lanes = lanes + pad[e * stride:(e + 1) * stride]
    waves = _tree64(lanes.reshape(stride // 64, 64))
    t = waves[0]
    for w in waves[1:]:
        t = t + w
    return float(t)


class Solve(object):
    __slots__ = ('xhat', 'nu', 'decisions', 'margin', 'trials', 'feasible')


def onecons_basis(lam, qhat, r, relop, slo, ehi, vhat, tier='ld', stride=64, small=False, tol=SEC_TOL, exact=False):
    """onecons_qcqp in a basis for one pair; see the module docstring.  relop: '<=' or '=='.  exact: phi and xhat in rational
    arithmetic (fractions.Fraction) -- tiny cases only."""
    f64 = tier in ('seq', 'kernel')
    if exact:
        conv = lambda a: [fractions.Fraction(float(t)) for t in np.asarray(a, dtype=np.float64)]
        L, Q, V, rr = conv(lam), conv(qhat), conv(vhat), fractions.Fraction(float(r))
    else:
        T = np.float64 if f64 else LD
        L, Q, V, rr = np.asarray(lam, dtype=T), np.asarray(qhat, dtype=T), np.asarray(vhat, dtype=T), T(r)
    rows = len(L)
    nz = np.asarray(lam, dtype=np.float64) != 0.0

    def value(x):                                          # (phi, scale) of a point in the basis
        if exact:
            a = sum(l * t * t for l, t in zip(L, x)); b = sum(q * t for q, t in zip(Q, x))
            sc = sum(abs(l) * t * t for l, t in zip(L, x)) + sum(abs(q * t) for q, t in zip(Q, x)) + abs(rr)
            return a + b + rr, sc
        ta, tb = L * (x * x), Q * x
        sc = float(np.sum(np.abs(ta)) + np.sum(np.abs(tb)) + abs(rr))
        if not f64:
            return np.sum(ta) + np.sum(tb) + rr, sc
        if small:                                          # admm_small_solve: p += lam x^2 + qhat x
            p = 0.0
            for e in range(rows):
                p = p + (ta[e] + tb[e])
            return p + rr, sc
        if tier == 'seq':
            return (_sum_seq(ta) + _sum_seq(tb)) + rr, sc
        return (_sum_kernel(ta, stride) + _sum_kernel(tb, stride)) + rr, sc

    def xh(nu):
        if exact:
            nuq = fractions.Fraction(float(nu))
            return [-(nuq * q - 2 * v) / (2 * (1 + nuq * l)) for l, q, v in zip(L, Q, V)]
        nuT = T(nu)
        num = -(nuT * Q - 2 * V)
        den = 2 * (1 + nuT * L)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            return np.where(nz, num / den, num * T(0.5))

    out = Solve()
    out.trials = 0
    margins = []

    def sign_at(x):
        p, sc = value(x)
        out.trials += 1
        margins.append(abs(float(p)) / sc if sc > 0 else np.inf)
        return int(p > 0) - int(p < 0)

    dec = []
    out.feasible = False
    if relop == '<=':                                      # the early return (utilities.py:157-158) is a decision like any other
        if sign_at(V) <= 0:
            out.xhat, out.nu, out.feasible = V, 0.0, True
            out.decisions, out.margin = 'F', min(margins)
            return out
    s, e = float(slo), float(ehi)
    guard = 0
    if s == -np.inf:
        s = -1.
        while sign_at(xh(s)) <= 0:
            s *= 2.; dec.append('a'); guard += 1
            assert guard < 200, 'open bracket start never closes: not a case for a test'
    if e == np.inf:
        e = 1.
        while sign_at(xh(e)) >= 0:
            e *= 2.; dec.append('b'); guard += 1
            assert guard < 400, 'open bracket end never closes: not a case for a test'
    while e - s > tol:
        mid = (s + e) / 2.
        p = sign_at(xh(mid))
        if p > 0:
            s = mid; dec.append('>')
        elif p < 0:
            e = mid; dec.append('<')
        else:
            s = e = mid; dec.append('0')
            break
    out.nu = (s + e) / 2.
    out.xhat = xh(out.nu)
    out.decisions, out.margin = ''.join(dec), min(margins)
    return out


def brackets(lam):
    """admm_brackets / utilities.py:176-180 per row of lam (m, rows), with the same float64 expression -1. / l."""
    lam = np.asarray(lam, dtype=np.float64)
    with np.errstate(divide='ignore'):
        inv = -1.0 / lam
    return np.where(lam > 0, inv, -np.inf).max(axis=1), np.where(lam < 0, inv, np.inf).min(axis=1)


def cancellation(lam, nu):
    l = np.asarray(lam, dtype=LD) * LD(nu)
    return float(np.max((1 + np.abs(l)) / np.abs(1 + l)))


def xhat_bound(lam, qhat, vhat, nu, e_v=0.0, feasible=False, e_q=0.0, yardstick=False):
    """Per element: the most a float64 evaluation (device or host) of xhat(nu) can differ from the longdouble one.  e_v, e_q: what
    the evaluation's own vhat and qhat may be off by (an error of qhat enters num as |nu| e_q)."""
    if feasible:
        return np.asarray(e_v, dtype=np.float64) + np.zeros(len(lam))
    L, Q, V, nuL = np.asarray(lam, dtype=LD), np.asarray(qhat, dtype=LD), np.asarray(vhat, dtype=LD), LD(nu)
    num, den = -(nuL * Q - 2 * V), 2 * (1 + nuL * L)
    x = np.abs(num / den)
    ev = np.asarray(e_v, dtype=LD) + np.abs(nuL) * np.asarray(e_q, dtype=LD) / 2

    def at(u, ev):
        e_num = u * (1 + u) * np.abs(nuL * Q) + u * np.abs(num)
        C = (1 + np.abs(nuL * L)) / np.abs(1 + nuL * L)
        r_den = np.where(L != 0, u * (1 + u) * (C + 1), 0)
        r_div = R_DIV * u
        return (e_num + 2 * ev) / np.abs(den) * (1 + r_den + r_div) / (1 - r_den) + x * (r_den / (1 - r_den) + r_div)

    if yardstick:                                          # the longdouble tier against exact arithmetic
        return np.asarray(at(LD(ULD), 0 * ev), dtype=np.float64)
    return np.asarray(at(LD(U), ev) + at(LD(ULD), 0 * ev), dtype=np.float64)


# ----------------------------------------------------------------------------------------------- spectra
SPECTRA = ('zero', 'onepos', 'oneneg', 'both', 'hi', 'last', 'qzero', 'feasible', 'both_le')


def spectrum(kind, rows, rs, geom):
    """(lam, qhat, relop, rmode) of one constraint.  rmode: 'any' (r drawn), 'neg' / 'pos' (sign that keeps a one-row constraint
    solvable), 'out' (every point of the population infeasible), 'in' (every point feasible)."""
    lam = np.zeros(rows)
    qhat = rs.randn(rows)
    mag = lambda k: rs.uniform(0.5, 2.0, size=k) * rs.choice([-1.0, 1.0], size=k)
    if kind == 'zero':                                     # 1. a linear constraint: both bracket ends by doubling
        return lam, qhat, '==', 'any'
    if kind in ('onepos', 'oneneg'):                       # 2, 3. one eigenvalue; half of the other coordinates untouched
        j = int(rs.randint(rows))
        lam[j] = rs.uniform(0.5, 2.0) * (1.0 if kind == 'onepos' else -1.0)
        if rows == 1:
            return lam, qhat, '==', 'neg' if kind == 'onepos' else 'pos'
        off = rs.rand(rows) < 0.5
        keep = [t for t in range(rows) if t != j]
        off[keep[0]] = False                               # a linear direction stays: the constraint is feasible
        qhat[off] = 0.0
        return lam, qhat, '<=', 'out'
    if kind in ('both', 'both_le', 'qzero', 'feasible'):   # 4. both signs, both ends finite; 7. qhat = 0; the feasible '<='
        lam = mag(rows)
        if rows >= 2:
            lam[0], lam[rows - 1] = abs(lam[0]), -abs(lam[rows - 1])
        if kind == 'qzero':
            qhat[:] = 0.0
            if rows == 1:
                return lam, qhat, '==', 'neg' if lam[0] > 0 else 'pos'
        rmode = {'both': 'any', 'qzero': 'any', 'both_le': 'out', 'feasible': 'in'}[kind]
        if rows == 1 and kind == 'both':                   # one row: real roots
            rmode = 'neg' if lam[0] > 0 else 'pos'
        return lam, qhat, {'both': '==', 'qzero': '==', 'both_le': '<=', 'feasible': '<='}[kind], rmode
    epl, stride = geom
    if kind == 'hi':                                       # 5. nonzero only in the upper half of the element slots
        sel = np.arange(rows) >= (epl // 2) * stride
        relop = '<='
    else:                                                  # 6. nonzero only in the last (partial) slot
        sel = np.arange(rows) >= ((rows - 1) // stride) * stride
        relop = '=='
    assert sel.any() and not sel.all(), (kind, rows, geom)
    lam[sel] = mag(int(sel.sum()))
    return lam, qhat, relop, 'out' if relop == '<=' else 'any'


def pick_r(rmode, lam, qhat, V, rs):
    """r of a constraint given the population in its basis, V (rows, R)."""
    g = lam.dot(V * V) + qhat.dot(V)
    size = 1.0 + np.abs(lam).dot(V * V).mean() + np.abs(qhat).dot(np.abs(V)).mean()
    if rmode == 'any':
        return float(rs.randn() * 0.5 * size)
    if rmode == 'neg':
        return -float(rs.uniform(0.5, 1.5))
    if rmode == 'pos':
        return float(rs.uniform(0.5, 1.5))
    if rmode == 'out':
        return float(0.05 * size - g.min())
    return float(-0.05 * size - g.max())                   # 'in'


# ----------------------------------------------------------------------------------------------- section A
class ACase(object):
    """One engine of section A: rows basis rows per constraint, m constraints with the spectra `kinds`, R points."""

    def __init__(self, rows, kinds, dense, seed, n=None, R=17):
        self.rows, self.kinds, self.dense, self.seed, self.R = rows, tuple(kinds), dense, seed, R
        self.n = (n if n is not None else rows) if not dense else 40
        self.m = len(kinds)
        self.lowrank = True
        self.expected = secular_instantiation(rows, True)

    @property
    def id(self):
        return '%s%d-%s' % ('dense' if self.dense else 'perm', self.rows, '+'.join(self.kinds))

    def build(self):
        rs = np.random.RandomState(self.seed)
        n, m, rows, R = self.n, self.m, self.rows, self.R
        geom = wave_geometry(rows, True)
        self.Z = rs.randn(n, R) * 10.0 ** rs.uniform(-0.5, 0.5, size=R)
        self.lam, self.qhat = np.zeros((m, rows)), np.zeros((m, rows))
        self.r, self.relop = np.zeros(m), []
        if self.dense:
            self.Bv = np.stack([np.linalg.qr(rs.randn(n, rows))[0].T for _ in range(m)])      # orthonormal rows, nothing unit about them
            self.perm = self.sgn = None
        else:
            self.perm = np.stack([rs.permutation(n)[:rows] for _ in range(m)])
            self.sgn = rs.choice([-1.0, 1.0], size=(m, rows))
            self.Bv = None
        self.V = np.zeros((m, rows, R), dtype=LD)
        for k, kind in enumerate(self.kinds):
            lam, qhat, relop, rmode = spectrum(kind, rows, rs, geom)
            Vk = self.vhat(k)
            self.lam[k], self.qhat[k] = lam, qhat
            self.r[k] = pick_r(rmode, lam, qhat, np.asarray(Vk, dtype=np.float64), rs)
            self.relop.append(relop)
            self.V[k] = Vk
        self.slo, self.ehi = brackets(self.lam)
        return self

    def vhat(self, k):
        """B_k Z: exact for a signed permutation, longdouble otherwise."""
        if self.dense:
            return np.asarray(self.Bv[k], dtype=LD).dot(np.asarray(self.Z, dtype=LD))
        return np.asarray(self.sgn[k][:, None] * self.Z[self.perm[k]], dtype=LD)

    def basis(self):
        """(m, rows, n) float64 for admm_set_basis."""
        if self.dense:
            return self.Bv
        B = np.zeros((self.m, self.rows, self.n))
        for k in range(self.m):
            B[k, np.arange(self.rows), self.perm[k]] = self.sgn[k]
        return B

    def funcs(self):
        """The problem the bases belong to: P_k = B_k' diag(lam_k) B_k, q_k = B_k' qhat_k (sparse for a permutation)."""
        n = self.n
        out = [(sp.identity(n, format='csr'), np.zeros(n), 0.0, None)]
        for k in range(self.m):
            if self.dense:
                B = self.Bv[k]
                P = (B.T * self.lam[k]).dot(B)
                q = B.T.dot(self.qhat[k])
                out.append(((P + P.T) / 2., q, float(self.r[k]), self.relop[k]))
            else:
                d = np.zeros(n); q = np.zeros(n)
                d[self.perm[k]] = self.lam[k]
                q[self.perm[k]] = self.sgn[k] * self.qhat[k]
                out.append((sp.diags(d, format='csr'), q, float(self.r[k]), self.relop[k]))
        return out

    def solve(self, k, c, tier='ld'):
        geom = wave_geometry(self.rows, True)
        v = self.V[k][:, c]
        if tier != 'ld' and self.dense:                    # a float64 tier forms B z itself, in float64
            v = self.Bv[k].dot(self.Z[:, c])
        return onecons_basis(self.lam[k], self.qhat[k], self.r[k], self.relop[k], self.slo[k], self.ehi[k], v, tier=tier,
                             stride=geom[1] if geom else 64, small=geom is None)

    def e_v(self, k, c):
        if not self.dense:
            return np.zeros(self.rows)
        return gamma(self.n) * np.abs(self.Bv[k]).dot(np.abs(self.Z[:, c]))

    def reference(self, k):
        """The longdouble projection of every point onto constraint k: dict(x (n, R) longdouble, bound (n, R), untouched (n,) mask of
        coordinates the constraint must leave bit for bit, decisions, margin, cancel)."""
        n, R, rows = self.n, self.R, self.rows
        X, Bd = np.zeros((n, R), dtype=LD), np.zeros((n, R))
        decs, margin, cancel = [], np.inf, 1.0
        Zl = np.asarray(self.Z, dtype=LD)
        for c in range(R):
            sv = self.solve(k, c)
            ev = self.e_v(k, c)
            ex = xhat_bound(self.lam[k], self.qhat[k], self.V[k][:, c], sv.nu, ev, sv.feasible)
            d = np.asarray(sv.xhat, dtype=LD) - self.V[k][:, c]
            dabs = np.asarray(np.abs(d), dtype=np.float64)
            ed = ex + ev + U * (dabs + ex + ev)
            if self.dense:
                Bk = self.Bv[k]
                x = Zl[:, c] + np.asarray(Bk, dtype=LD).T.dot(d)
                eb = np.abs(Bk).T.dot(ed) + gamma(rows) * np.abs(Bk).T.dot(dabs + ed)
            else:
                x = Zl[:, c].copy()
                x[self.perm[k]] += self.sgn[k] * d
                eb = np.zeros(n)
                eb[self.perm[k]] = ed + gamma(1) * (dabs + ed)
            if sv.feasible:
                x, eb = Zl[:, c], np.zeros(n)              # the point itself, bit for bit
            X[:, c] = x
            Bd[:, c] = eb + U * (np.asarray(np.abs(x), dtype=np.float64) + eb)
            if sv.feasible:
                Bd[:, c] = 0.0
            decs.append(sv.decisions)
            margin = min(margin, sv.margin)
            if not sv.feasible:
                cancel = max(cancel, cancellation(self.lam[k], sv.nu))
        untouched = np.zeros(n, dtype=bool)
        if not self.dense:
            untouched[:] = True
            moved = (self.lam[k] != 0) | (self.qhat[k] != 0)
            untouched[self.perm[k][moved]] = False
        return dict(x=X, bound=Bd, untouched=untouched, decisions=decs, margin=margin, cancel=cancel)


def _groups(m, rows):
    if rows == 1:
        return [('zero', 'onepos', 'oneneg'), ('feasible', 'qzero', 'both')]
    if rows <= 9:
        return [('zero', 'onepos', 'both'), ('oneneg', 'qzero', 'feasible')]
    if m == 3:
        return [('zero', 'onepos', 'both'), ('oneneg', 'hi', 'last'), ('qzero', 'feasible', 'both_le')]
    if m == 2:
        return [('both', 'hi'), ('last', 'zero'), ('feasible', 'oneneg')]
    return [('both',), ('hi',)]


# rows at both sides of every switch of admm_launch_secular; (rows, m)
A_SMALL_ROWS = (1, 2, 4, 8, 9)
A_SWITCHES = ((128, 129), (256, 257), (512, 513), (1024, 1025), (2048, 2049), (4096, 4097), (8192, 8193))
A_PERM_ROWS = tuple(r for pair in A_SWITCHES for r in pair)


def a_m(rows):
    return 3 if rows <= 1025 else (2 if rows <= 4097 else 1)


def a_cases():
    out = []
    for rows in A_SMALL_ROWS:
        for g, kinds in enumerate(_groups(3, rows)):
            out.append(ACase(rows, kinds, True, 1000 * rows + g))
    for rows in A_PERM_ROWS:
        groups = _groups(a_m(rows), rows)
        if rows == 8192:
            groups = groups[:1]                            # the hi spectrum of <32, 4> needs rows > 4096: covered at 4097
        for g, kinds in enumerate(groups):
            out.append(ACase(rows, kinds, False, 1000 * rows + g))
    return out


A_CASES = a_cases()
# real eigenpairs of dense indefinite constraints through qcqpmi_admm_set_eig (full basis, lowrank = 0)
A_EIG_NS = (129, 257)


def eig_problem(n, m=2, seed=0, R=17):
    """Dense indefinite constraints ('==' and an infeasible '<='), their eigh pairs, a population."""
    rs = np.random.RandomState(7000 + n + seed)
    funcs = [(np.eye(n), np.zeros(n), 0.0, None)]
    Z = rs.randn(n, R)
    for k in range(m):
        A = rs.randn(n, n) / np.sqrt(n)
        P = (A + A.T) / 2.
        q = rs.randn(n)
        g = np.einsum('ir,ij,jr->r', Z, P, Z) + q.dot(Z)
        relop = '==' if k % 2 == 0 else '<='
        r = float(rs.randn()) if relop == '==' else float(1.0 - g.min())
        funcs.append((P, q, r, relop))
    lm = np.zeros((m, n)); Q = np.zeros((m, n, n))
    for k in range(m):
        lm[k], Q[k] = np.linalg.eigh(funcs[k + 1][0])
    return funcs, lm, Q, Z


def qhat_like_set_eig(Qk, q):
    """qcqpmi_admm_set_eig: acc += Q[i][j] * q[i], i ascending, unfused float64."""
    return np.add.accumulate(Qk * q[:, None], axis=0)[-1]


def eig_reference(funcs, lm, Q, Z, k):
    """Full-basis projection onto constraint k (0-based) in longdouble with its bound; vhat = Q' z."""
    n, R = Z.shape
    P, q, r, relop = funcs[k + 1]
    Qk = Q[k]
    qh = qhat_like_set_eig(Qk, q)
    slo, ehi = brackets(lm[k][None])
    Ql, Zl = np.asarray(Qk, dtype=LD), np.asarray(Z, dtype=LD)
    Vh = Ql.T.dot(Zl)
    X, Bd, Bo = np.zeros((n, R), dtype=LD), np.zeros((n, R)), np.zeros((n, R))
    e_q = gamma(n) * np.abs(Qk).T.dot(np.abs(q))
    margin, cancel, decs = np.inf, 1.0, []
    for c in range(R):
        sv = onecons_basis(lm[k], qh, r, relop, slo[0], ehi[0], Vh[:, c], stride=wave_geometry(n, False)[1])
        ev = gamma(n) * np.abs(Qk).T.dot(np.abs(Z[:, c]))
        ex = xhat_bound(lm[k], qh, Vh[:, c], sv.nu, ev, sv.feasible)
        xa = np.asarray(np.abs(sv.xhat), dtype=np.float64)
        X[:, c] = Ql.dot(np.asarray(sv.xhat, dtype=LD))
        Bd[:, c] = np.abs(Qk).dot(ex) + gamma(n) * np.abs(Qk).dot(xa + ex)
        eo = xhat_bound(lm[k], qh, Vh[:, c], sv.nu, ev, sv.feasible, e_q=e_q)      # an evaluation that forms qhat in another order
        Bo[:, c] = np.abs(Qk).dot(eo) + gamma(n) * np.abs(Qk).dot(xa + eo)
        margin = min(margin, sv.margin); decs.append(sv.decisions)
        if not sv.feasible:
            cancel = max(cancel, cancellation(lm[k], sv.nu))
    return dict(x=X, bound=Bd, bound_other=Bo, margin=margin, cancel=cancel, decisions=decs)


# ----------------------------------------------------------------------------------------------- section B
# (n, m, R): the two products as a linear operator, x = Q_k (Q_k' z)
B_FIRST_ONLY = smallest_first_product_big()
B_CASES = [
    (40, 3, 1),            # one column, one partial tile; 8 hat row blocks (7.5 of them real)
    (100, 3, 17),          # 19 hat row blocks, 7 n blocks, two tiles: nothing a multiple of 4
    (256, 1, 16384),       # the smallest shape at which BOTH products take gemm_pk_kernel
    (270, 1, 10923),       # gemm_pk_kernel with 17 row blocks, 17 k-blocks and 683 tiles: every edge ragged
    B_FIRST_ONLY,          # the first product alone on gemm_pk_kernel
]


def gemm_problem(n, m, R, seed=0):
    rs = np.random.RandomState(9000 + n + m + seed)
    Q = rs.randn(m, n, n) / np.sqrt(n)
    Z = rs.randn(n, R) * 10.0 ** rs.uniform(-1.0, 1.0, size=R)
    funcs = [(sp.identity(n, format='csr'), np.zeros(n), 0.0, None)]
    for k in range(m):
        funcs.append((sp.csr_matrix((n, n)), np.zeros(n), -1.0, '<='))      # always feasible: onecons returns Q (Q' z)
    return funcs, Q, Z


def gemm_bound(Qk, Z):
    n = Qk.shape[0]
    g = gamma(n)
    return (2 * g + g * g) * np.abs(Qk).dot(np.abs(Qk).T.dot(np.abs(Z)))


def gemm_check(X, Qk, Z, sample):
    """Worst error / bound of X against Q (Q' Z): every column against the float64 product (both sides carry the bound: 2 x), the
    sampled columns against longdouble (1 x).  Returns (worst all columns, worst sampled)."""
    bound = gemm_bound(Qk, Z)
    ref = Qk.dot(Qk.T.dot(Z))
    w_all = float(np.max(np.abs(X - ref) / (2 * bound)))
    Ql = np.asarray(Qk, dtype=LD)
    refl = Ql.dot(Ql.T.dot(np.asarray(Z[:, sample], dtype=LD)))
    w_ld = float(np.max(np.asarray(np.abs(X[:, sample] - refl), dtype=np.float64) / bound[:, sample]))
    return w_all, w_ld


def sample_columns(R):
    return sorted(set(c for c in (0, 1, 15, 16, 17, R // 2, R - 17, R - 16, R - 2, R - 1) if 0 <= c < R))


# ----------------------------------------------------------------------------------------------- section D
APPLY_PS = (1, 15, 16, 17, 64)
APPLY_NS = (33, 40)
ZSOLVER_NS = (16, 17, 130)


def apply_bound(P, V):
    """admm_apply_constraints_kernel: two fma chains over the even and the odd j and their sum -- a product passes through at most
    ceil(n / 2) + 1 roundings.  P (m, n, n); V (n, p) shared or (m, n, p)."""
    n = P.shape[-1]
    Va = np.abs(V)
    A = np.einsum('kij,jc->kic', np.abs(P), Va) if V.ndim == 2 else np.einsum('kij,kjc->kic', np.abs(P), Va)
    return gamma((n + 1) // 2 + 1) * A


# ----------------------------------------------------------------------------------------------- section C
class CCase(object):
    """One problem of section C: 1, 2 and 3 iterations of qcqpmi_admm_run against the oracle's improve_admm.
    basis: 'reduced' (rp rows per constraint through admm_set_basis), 'full' (eigh pairs through admm_set_eig) or 'unit'
    (Boolean least squares through QCQPForm.unit_bases).  p0: 'diag' | 'dense'; solver: 'diag' | 'host' | 'device'.
    debug: bits of qcqpmi_debug_profile >> 4 (2: three launches instead of the unit step, 4: f0 through the product with P0)."""

    def __init__(self, name, n, m, R, basis='reduced', rp=2, p0='diag', solver='diag', debug=0, viol_lim=1e4, feasible_starts=0,
                 all_le=False, seed=0):
        self.name, self.n, self.m, self.R, self.basis, self.rp = name, n, m, R, basis, rp
        self.p0, self.solver, self.debug, self.viol_lim, self.feasible_starts, self.all_le = p0, solver, debug, viol_lim, feasible_starts, all_le
        self.seed = seed
        self.rows = rp if basis == 'reduced' else (1 if basis == 'unit' else n)
        self.lowrank = basis != 'full'

    @property
    def id(self):
        return self.name

    def geometry(self):
        return geometry(self.n, self.m, self.rows, self.lowrank, self.R, unit=self.basis == 'unit')

    def build(self):
        rs = np.random.RandomState(4000 + self.seed + 7 * self.n + 13 * self.m + self.R)
        n, m, R = self.n, self.m, self.R
        self.rho = 1.0
        if self.p0 == 'diag':
            d = rs.uniform(0.5, 2.0, size=n)
            P0 = sp.diags(d, format='csr')
            self.P0 = np.diag(d)
        else:
            A = rs.randn(n, n)
            self.P0 = A.T.dot(A) / n + 0.5 * np.eye(n)
            self.P0 = (self.P0 + self.P0.T) / 2.
            P0 = self.P0
        q0 = rs.randn(n)
        funcs = [(P0, q0, float(rs.randn()), None)]
        self.X0 = rs.randn(n, R) * 1.5
        lm = np.zeros((m, n)); Q = np.zeros((m, n, n))
        if self.basis == 'unit':                           # x_i^2 = 1 for every coordinate: m = n
            assert m == n
            for i in range(n):
                d = np.zeros(n); d[i] = 1.0
                funcs.append((sp.diags(d, format='csr'), np.zeros(n), -1.0, '=='))
                lm[i, n - 1] = 1.0                         # what LAPACK returns for e_i e_i': eigenvalues {0, .., 0, 1}, unit eigenvectors
                order = [j for j in range(n) if j != i] + [i]
                Q[i] = np.eye(n)[:, order]
            self.lam = self.Bv = self.qhat = None
        elif self.basis == 'full':
            for k in range(m):
                A = rs.randn(n, n) / np.sqrt(n)
                P = (A + A.T) / 2.
                relop = '<=' if (self.all_le or k % 2) else '=='
                funcs.append((P, rs.randn(n), -abs(float(rs.randn())) - 0.2 if relop == '<=' else float(rs.randn()), relop))
                lm[k], Q[k] = np.linalg.eigh(P)
            self.lam = self.Bv = self.qhat = None
        else:
            rp = self.rp
            self.lam, self.qhat, self.Bv = np.zeros((m, rp)), np.zeros((m, rp)), np.zeros((m, rp, n))
            for k in range(m):
                Qc = np.linalg.qr(rs.randn(n, rp), mode='complete')[0]
                B = Qc[:, :rp].T
                lam = rs.uniform(0.5, 2.0, size=rp) * rs.choice([-1.0, 1.0], size=rp)
                if rp >= 2:
                    lam[0], lam[rp - 1] = abs(lam[0]), -abs(lam[rp - 1])
                if rp > 4:
                    lam[2:rp - 2] = 0.0                    # (padding rows of a rank-4 constraint)
                qhat = rs.randn(rp)
                relop = '<=' if (self.all_le or k % 2) else '=='
                r = -abs(float(rs.randn())) - 0.2 if relop == '<=' else float(rs.randn())
                P = (B.T * lam).dot(B)
                funcs.append(((P + P.T) / 2., B.T.dot(qhat), r, relop))
                self.lam[k], self.qhat[k], self.Bv[k] = lam, qhat, B
                lm[k, :rp] = lam
                Q[k] = np.concatenate([B.T, Qc[:, rp:]], axis=1)
        if self.feasible_starts:                           # every constraint is a '<=' with r < 0: small points are feasible
            assert self.all_le
            cols = np.arange(R)[::max(1, R // self.feasible_starts)][:self.feasible_starts]
            self.X0[:, cols] *= 1e-3
            self.feasible_cols = cols
        self.funcs, self.lm, self.Q = funcs, np.ascontiguousarray(lm), np.ascontiguousarray(Q)
        self.Minv = np.linalg.inv(2. * (self.P0 + self.rho * m * np.eye(n))) if self.solver == 'host' else None
        return self


def oracle_admm(prob, x0, rho, num_iters, phase1, viol_lim=1e4, tol=1e-2):
    """improve_admm (qcqp.py:254-285) through the oracle's phases, and the iteration counts qcqpmi_admm_run reports for the same
    trajectory.  The device counts the iterations that did NOT stop and knows the violation of z_t in iteration t itself (the
    secular kernel evaluates it); the reference tests z_t at the top of iteration t + 1 and counts a stopping iteration of phase 2.
    Both are read off a run with one more iteration: a stop inside the first num_iters iterations shows there as a shorter count."""
    it1 = 0
    if phase1:
        z1, _ = prob.admm_phase1(x0, tol, num_iters)
        _, ext = prob.admm_phase1(x0, tol, num_iters + 1)
        it1 = 0 if ext == 0 else (ext - 1 if ext <= num_iters else num_iters)
        x1 = x0 if prob.better(x0, z1) == 1 else z1
    else:
        x1 = x0
    z2, _ = prob.admm_phase2(x1, rho, tol, num_iters, viol_lim)
    _, ext = prob.admm_phase2(x1, rho, tol, num_iters + 1, viol_lim)
    it2 = ext - 1 if ext <= num_iters else num_iters
    x2 = x1 if prob.better(x1, z2) == 1 else z2
    return x2, it1, it2


C_ITERS = (1, 2, 3)
C_CASES = [
    CCase('red2-R17', 20, 3, 17, rp=2),
    CCase('red4-R15', 20, 3, 15, rp=4),
    CCase('red8-R33-hostMinv', 24, 3, 33, rp=8, p0='dense', solver='host'),
    CCase('red9-wave-R17', 24, 3, 17, rp=9),
    CCase('red2-R1', 20, 3, 1, rp=2),
    CCase('full-deviceMinv', 24, 3, 17, basis='full', p0='dense', solver='device'),
    CCase('full-n48-m6-zs2', 48, 6, 17, basis='full'),
    CCase('unit-step', 24, 24, 17, basis='unit', p0='dense', solver='device'),
    CCase('unit-three-launches', 24, 24, 17, basis='unit', p0='dense', solver='device', debug=2),
    CCase('unit-diag', 24, 24, 15, basis='unit'),
    CCase('m15', 20, 15, 17, rp=2),
    CCase('m16-lds', 20, 16, 17, rp=2),
    CCase('m17', 20, 17, 17, rp=2),
    CCase('dense-f0-solve', 20, 3, 17, rp=2, p0='dense', solver='host'),
    CCase('dense-f0-product', 20, 3, 17, rp=2, p0='dense', solver='host', debug=4),
    CCase('n272-zs1', 272, 3, 17, rp=2),
    CCase('m32-rp8-zs2', 40, 32, 17, rp=8),
    CCase('feasible-starts', 20, 3, 33, rp=2, all_le=True, feasible_starts=5),
    CCase('viol-lim', 20, 3, 17, rp=2, viol_lim=0.5, seed=1),
]
C_TOL = 1e-9


# ----------------------------------------------------------------------------------------------- the inverse, section D
def _as_ints(A, k):
    """A 2^k as Python integers (exact; k large enough for every entry)."""
    out = np.empty(A.shape, dtype=object)
    for idx, v in np.ndenumerate(np.asarray(A, dtype=np.float64)):
        s = float(np.ldexp(v, k))
        assert s == int(s)
        out[idx] = int(s)
    return out


def _shift(A):
    nz = np.abs(A[A != 0])
    return 53 - int(np.floor(np.log2(nz.min()))) if nz.size else 0


def inverse_yardstick(M):
    """M^-1 in longdouble, every entry good to a few units of 2^-64 relative to ITSELF plus |M^-1| R^2 with R ~ 1e-18: two Newton
    steps X <- X + X (I - M X) from the float64 inverse with the residual formed EXACTLY (integer arithmetic on the bits) -- a
    residual formed in longdouble carries n 2^-64 |M| |X|, which is more than an entry of size 1e-7 can afford."""
    n = M.shape[0]
    kM = _shift(M)
    Mi = _as_ints(M, kM)
    X = np.asarray(np.linalg.inv(M), dtype=LD)
    for _ in range(2):
        hi = np.asarray(X, dtype=np.float64)
        lo = np.asarray(X - hi, dtype=np.float64)          # exact: 64 mantissa bits split into 53 + 11
        kX = max(_shift(hi), _shift(lo))
        Xi = _as_ints(hi, kX) + _as_ints(lo, kX)
        Ri = np.eye(n, dtype=object) * (1 << (kM + kX)) - Mi.dot(Xi)
        R = np.array([[LD(int(v)) for v in row] for row in Ri], dtype=LD) / LD(2.0) ** (kM + kX)
        X = X + X.dot(R)
    return X, float(np.max(np.abs(R)))


# ----------------------------------------------------------------------------------------------- section C on the host
_C_MARGINS = {}


def c_margins(case):
    """Every onecons_qcqp call of every run of a section-C case (num_iters 1, 2, 3, phase 1 on and off; the shorter runs are
    prefixes of the longer ones), replayed on the host in the basis the DEVICE uses: the longdouble tier and both float64 orders
    must take the same decisions and stay inside xhat_bound.  Returns (calls, smallest margin, largest cancellation factor,
    worst float64 error / bound)."""
    key = (case.basis, case.n, case.m, case.R, case.rp, case.p0, case.viol_lim, case.all_le, case.feasible_starts, case.seed)
    if key in _C_MARGINS:                                  # cases that differ in a debug switch or the z-solver share their problem
        return _C_MARGINS[key]
    n, m, R, rho = case.n, case.m, case.R, case.rho
    Ps = [np.asarray(f[0].todense()) if sp.issparse(f[0]) else np.asarray(f[0]) for f in case.funcs]
    qs = [np.asarray(f[1], dtype=np.float64) for f in case.funcs]
    rsv = [float(f[2]) for f in case.funcs]
    rel = [f[3] for f in case.funcs]
    if case.basis == 'reduced':
        lam, qh, Bs = case.lam, case.qhat, case.Bv
    elif case.basis == 'unit':
        lam = np.array([[Ps[k + 1][k, k]] for k in range(m)]); qh = np.array([[qs[k + 1][k]] for k in range(m)])
        Bs = np.zeros((m, 1, n)); Bs[np.arange(m), 0, np.arange(m)] = 1.0
    else:
        lam, Bs = case.lm, np.stack([case.Q[k].T for k in range(m)])
        qh = np.stack([qhat_like_set_eig(case.Q[k], qs[k + 1]) for k in range(m)])
    rows = lam.shape[1]
    slo, ehi = brackets(lam)
    geom = wave_geometry(rows, case.lowrank)
    stat = dict(calls=0, margin=np.inf, cancel=1.0, worst=0.0)
    Minv = np.linalg.inv(2. * (case.P0 + rho * m * np.eye(n)))

    def fval(k, x):
        return x.dot(Ps[k].dot(x)) + qs[k].dot(x) + rsv[k]

    def maxviol(x):
        return max((abs(fval(k, x)) if rel[k] == '==' else max(fval(k, x), 0.0)) for k in range(1, m + 1))

    def better(x1, x2):
        v1, v2 = int(maxviol(x1) / 1e-4), int(maxviol(x2) / 1e-4)
        if v1 != v2:
            return x1 if v1 < v2 else x2
        return x1 if fval(0, x1) < fval(0, x2) else x2

    def onecons(k, v):
        B = Bs[k]
        vl = np.asarray(B, dtype=LD).dot(np.asarray(v, dtype=LD))
        vf = B.dot(v)
        args = (lam[k], qh[k], rsv[k + 1], rel[k + 1], slo[k], ehi[k])
        kw = dict(stride=geom[1] if geom else 64, small=geom is None)
        a = onecons_basis(*args, vl, tier='ld', **kw)
        ev = gamma(np.count_nonzero(B, axis=1).max()) * np.abs(B).dot(np.abs(v)) if case.basis != 'unit' else 0.0
        ex = xhat_bound(lam[k], qh[k], vl, a.nu, ev, a.feasible)
        for tier in ('seq', 'kernel'):
            b = onecons_basis(*args, vf, tier=tier, **kw)
            assert b.decisions == a.decisions and b.nu == a.nu, (case.id, k, tier)
            err = np.abs(np.asarray(b.xhat, dtype=LD) - a.xhat).astype(np.float64)
            assert np.all(err <= ex), (case.id, k, tier)
            if (ex > 0).any():
                stat['worst'] = max(stat['worst'], float(np.max(err[ex > 0] / ex[ex > 0])))
        stat['calls'] += 1
        stat['margin'] = min(stat['margin'], a.margin)
        if not a.feasible:
            stat['cancel'] = max(stat['cancel'], cancellation(lam[k], a.nu))
        if a.feasible:
            return v.copy()
        return v + B.T.dot(np.asarray(b.xhat, dtype=np.float64) - vf)      # x = v + B' (xhat - B v)

    def project(z, us):
        xs = np.stack([onecons(k, z + us[k]) for k in range(m)])
        return xs, us + (z[None] - xs)

    for c in range(R):
        x0 = case.X0[:, c]
        starts = [x0]
        xs, us, z = np.stack([x0] * m), np.zeros((m, n)), x0.copy()
        for t in range(max(C_ITERS)):                      # phase 1 (qcqp.py:195-212); x1 after 1, 2, 3 iterations
            if maxviol(z) < 1e-2:
                break
            z = (xs.sum(axis=0) - us.sum(axis=0)) / m
            xs, us = project(z, us)
            starts.append(better(x0, z))
        distinct = dict((x1.tobytes(), x1) for x1 in starts)
        for x1 in distinct.values():                       # phase 2 (qcqp.py:215-251) from every x1
            xs, us, last = np.stack([x1] * m), np.zeros((m, n)), None
            for t in range(max(C_ITERS)):
                z = Minv.dot(2. * rho * (xs.sum(axis=0) - us.sum(axis=0)) - qs[0])
                xs, us = project(z, us)
                if last is not None and np.linalg.norm(last - z) < 1e-2:
                    break
                last = z
                if maxviol(z) > case.viol_lim:
                    break
    _C_MARGINS[key] = stat
    return stat
