"""What tests/test_spectrum_lattice_cpu.py and tests/test_gpu_spectrum_lattice.py share (a plain module, no test in it): a lattice of
trust-region problems and ADMM setups whose SPECTRUM IS KNOWN EXACTLY, for the four kernels that rest on the two eigen-solvers.

exact_q            an orthogonal matrix of dyadic rationals with Q'Q == I in double arithmetic: a direct sum of Sylvester-Hadamard
                   blocks (64, 16, 4 scaled by 2^-3, 2^-2, 2^-1; 1 x 1 for the rest), rows and columns permuted, times ONE Householder
                   I - (2 / k) v v' with k = 2^j entries of v in {+1, -1} and zeros elsewhere.  Entries are multiples of 2^-6.
spectrum           seven spectra of small dyadic values (max |lam| / min nonzero |lam| <= 2^12; the cluster 1 + k 2^-40 is the one that
                   needs 40 bits), so that P0 = Q diag(lam) Q' is exact in double.
rhs                right-hand sides in the eigenbasis: gh of small integers (g = Q gh, q0 = 2 g), and for the diagonal tier a pair on
                   the two sides of the hard-case threshold 2^-46.
Tier A             Q = a permutation: the solvers rotate nothing (narrow 0 sweeps, wide 1), lam and gh reach the lanes exactly and
                   every decision of the secular stage is exact and known.  Tier B: the dense Q.
exact              the trust-region problem in the eigenbasis with the standard library alone: rationals for every decision (interior,
                   hard case, tau), decimal arithmetic at 80 digits for the root of the secular equation, which is CERTIFIED by a sign
                   change of psi - rho^2 across [sigma (1 - 1e-60), sigma (1 + 1e-60)] (a safeguarded Newton iteration finds it, plain
                   bisection if the certificate fails).
exact_minv         Q diag(1 / (2 (lam + rho m))) Q' entry by entry in integers (the weights carried to 2^-200, everything else exact),
                   rounded to double once.
The measured constants at the end are the worst figures of the NumPy restatements against these references over the whole lattice
(tests/test_spectrum_lattice_cpu.py asserts that they are not exceeded); the GPU test allows ten times each.
"""
import functools
import math
from decimal import Context, Decimal
from fractions import Fraction

import numpy as np

import spectral_batch_cases as sc

SIZES = (1, 2, 3, 4, 16, 31, 33, 63, 64)
SIZES_WIDE = (65, 66, 96, 127, 128)
SPECTRA = ('equal', 'multi', 'cluster', 'rank1', 'psd0', 'pm', 'two')
RHS = ('generic', 'zeroL', 'one', 'zero')
THRESHOLD = ('thr45', 'thr47')         # |gh_L| = 2^-45 |gh| (regular side) and 2^-47 |gh| (hard side): Tier A only
SEED = 5
Q_BITS = 6                             # every entry of exact_q is a multiple of 2^-Q_BITS
DEC = Context(prec=80)
SCALE_SIZES = (33, 64, 65, 128)        # the sizes of the power-of-two scaling checks
TINY, HUGE = 2.0 ** -600, 2.0 ** 520   # the squares of the entries underflow to 0.0 / overflow to inf
R0 = 0.5
# The sweep limit of every call on this lattice.  With REPEATED eigenvalues scattered over the diagonal the two-sided cyclic Jacobi of
# jacobi_small.h converges only linearly (a pair inside one eigenspace has a_pp - a_qq and a_pq of the same small order, so it turns
# by a large angle and carries the couplings to the other eigenspaces along): the NumPy restatement needs up to 56 sweeps to reach
# off(A) <= 1e-15 |A|_F on the Tier B matrices ('two' at n = 64; 43 at n = 33) and reports status 1 at the default of 30, with lam
# already within 6e-16 |A|_F.  The limit is an argument of the calls; 100 leaves the slowest case a factor of almost two.  The wide
# solver (one-sided, shifted) needs at most 15 on this lattice (20 on the device).
MAX_SWEEPS, TOL = 100, 1e-15


# ------------------------------------------------------------------ exact orthogonal matrices
def hadamard(k):
    H = np.ones((1, 1))
    while H.shape[0] < k:
        H = np.block([[H, H], [H, -H]])
    return H


@functools.lru_cache(maxsize=None)
def exact_q(n, seed=SEED):
    rs = np.random.RandomState(1000 * seed + n)
    Q = np.zeros((n, n))
    i = 0
    for size, scale in ((64, 2.0 ** -3), (16, 2.0 ** -2), (4, 2.0 ** -1)):
        while n - i >= size and n >= 4:
            Q[i:i + size, i:i + size] = hadamard(size) * scale
            i += size
    Q[np.arange(i, n), np.arange(i, n)] = 1.0
    Q = Q[rs.permutation(n)][:, rs.permutation(n)]
    k = 1
    while 2 * k <= min(n, 16):
        k *= 2
    v = np.zeros(n)
    v[rs.permutation(n)[:k]] = rs.choice([-1.0, 1.0], size=k)
    Q = Q - (2.0 / k) * np.outer(Q.dot(v), v)
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=None)
def perm_q(n, seed=SEED):
    """Tier A: eigen-index k sits at coordinate pi(k)."""
    pi = np.random.RandomState(2000 * seed + n).permutation(n)
    Q = np.zeros((n, n))
    Q[pi, np.arange(n)] = 1.0
    Q.setflags(write=False)
    return Q


# ------------------------------------------------------------------ spectra and right-hand sides
def spectrum(name, n):
    """lam by eigen-index (NOT sorted)."""
    if name == 'equal':
        return np.full(n, 2.0)
    if name == 'multi':           # the lowest eigenvalue -2 with multiplicity max(1, n // 3), ties among the others too
        mult = max(1, n // 3)
        rest = (-1.0, -0.5, 0.25, 1.0, 1.5, 3.0)
        return np.array([-2.0] * mult + [rest[j % 6] for j in range(n - mult)])
    if name == 'cluster':
        return 1.0 + np.arange(n) * 2.0 ** -40
    if name == 'rank1':
        lam = np.zeros(n)
        lam[n - 1] = 4.0
        return lam
    if name == 'psd0':
        return np.array([0.0] + [1.0 + (j % 5) for j in range(n - 1)])
    if name == 'pm':
        lam = []
        for j in range(n // 2):
            lam += [(1.0, 2.0, 4.0)[j % 3], -(1.0, 2.0, 4.0)[j % 3]]
        return np.array(lam + ([0.5] if n % 2 else []))
    if name == 'two':
        return np.where(np.arange(n) < n // 2, -1.0, 3.0)
    raise KeyError(name)


def rhs(name, lam, seed):
    """gh by eigen-index, or None where the family does not exist for this spectrum."""
    n = lam.size
    rs = np.random.RandomState(seed)
    low = lam == lam.min()
    gen = rs.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=n)
    if name == 'generic':
        return gen
    if name == 'zeroL':
        return np.where(low, 0.0, gen)
    if name == 'one':
        gh = np.zeros(n)
        gh[rs.randint(n)] = 2.0
        return gh
    if name == 'zero':
        return np.zeros(n)
    # the threshold pair: the hard rule is asked (lam_min <= 0 gives sigma_lo == 0 for both relops), the other components have norm 1
    # and sit at d_k >= 1, so psi_reg <= 1 <= rho^2; ONE component of the lowest eigenspace carries 2^-45 or 2^-47
    other = np.flatnonzero(~low)
    if lam.min() > 0.0 or other.size == 0:
        return None
    assert np.all(lam[other] - lam.min() >= 1.0)
    gh = np.zeros(n)
    if other.size >= 4:
        gh[rs.choice(other, size=4, replace=False)] = 0.5 * rs.choice([-1.0, 1.0], size=4)
    else:
        gh[other[0]] = -1.0
    gh[np.flatnonzero(low)[-1]] = 2.0 ** (-45 if name == 'thr45' else -47)
    return gh


# ------------------------------------------------------------------ the lattice
def _agg(cons, n):
    if cons == 'bool':            # x_i^2 == 1 (or <= 1): a = 1, beta = 0, rho^2 = n
        return np.concatenate([np.ones(n), np.zeros(n), [-float(n)]]), float(n)
    return np.concatenate([np.ones(n), -np.ones(n), [0.0]]), 0.25 * n         # x_i (x_i - 1) <= 0: h = -1/2, rho^2 = n / 4


@functools.lru_cache(maxsize=None)
def matrices(n):
    """{(tier, spectrum): (Q, lam, P0)} -- the 14 matrices of one size, shared by the trust-region cases and the setups."""
    out = {}
    for tier, Q in (('A', perm_q(n)), ('B', exact_q(n))):
        for name in SPECTRA:
            lam = spectrum(name, n)
            P0 = (Q * lam).dot(Q.T)
            P0 = 0.5 * (P0 + P0.T)
            P0.setflags(write=False)
            out[tier, name] = (Q, lam, P0)
    return out


@functools.lru_cache(maxsize=None)
def cases(n, relop):
    """The trust-region cases of one size and relop: a list of dictionaries (tier, spectrum, rhs, cons, Q, lam, gh, P0, q0, r0, agg,
    rho2, h).  Boolean constraints for both relops; the box [0, 1] (beta != 0) for '<=' (the cluster is left out there: q0 = 2 g -
    P0 1 would not be exact)."""
    out = []
    for (tier, name), (Q, lam, P0) in matrices(n).items():
        for cons in ('bool',) + (('box',) if relop == '<=' and name != 'cluster' else ()):
            agg, rho2 = _agg(cons, n)
            h = agg[n:2 * n] / 2.0
            for r, rname in enumerate(RHS + (THRESHOLD if tier == 'A' and cons == 'bool' else ())):
                gh = rhs(rname, lam, 100 * n + 10 * SPECTRA.index(name) + r)
                if gh is None:
                    continue
                g = Q.dot(gh)
                q0 = 2.0 * (g + P0.dot(h))
                out.append(dict(tier=tier, spectrum=name, rhs=rname, cons=cons, Q=Q, lam=lam, gh=gh, P0=P0, g=g, q0=q0, r0=R0, agg=agg,
                                rho2=rho2, h=h))
    return out


def case_id(c):
    return '%s-%s-%s-%s' % (c['tier'], c['spectrum'], c['rhs'], c['cons'])


def batch(n, relop):
    cs = cases(n, relop)
    return (cs, np.stack([c['P0'] for c in cs]), np.stack([c['q0'] for c in cs]), np.array([c['r0'] for c in cs]),
            np.stack([c['agg'] for c in cs]))


def boolean_funcs(n):
    """A context for the calls: n variables over m = n Boolean constraints."""
    return [(np.eye(n), np.zeros(n), 0.0, None)] + sc._cons(n, -1.0, 1.0, '==')


# ------------------------------------------------------------------ exact integer arithmetic on Q diag(w) Q'
def _congruence(Q, W):
    """sum_k W_k q_k q_k' 2^(2 Q_BITS) for Python integers W_k >= 0, as an object array of Python integers: the weights go in limbs of
    30 bits through int64 products (|Q 2^Q_BITS|^2 2^30 n < 2^63)."""
    Qi = np.rint(Q * 2.0 ** Q_BITS).astype(np.int64)
    assert np.array_equal(Qi / 2.0 ** Q_BITS, Q) and int(np.max(np.abs(Qi))) ** 2 * Q.shape[0] < 2 ** 32
    assert all(w >= 0 for w in W)
    total = np.zeros(Q.shape, dtype=object)
    shift = 0
    W = list(W)
    while any(W):
        limb = np.array([w & ((1 << 30) - 1) for w in W], dtype=np.int64)
        total = total + (Qi * limb).dot(Qi.T).astype(object) * (1 << shift)
        W = [w >> 30 for w in W]
        shift += 30
    return total


def rational_p0(Q, lam):
    """Q diag(lam) Q' as an object array of Fractions (lam: multiples of 2^-42 in [-2^12, 2^12])."""
    L = [Fraction(float(v)) * 2 ** 42 for v in lam]
    assert all(v.denominator == 1 for v in L)
    L = [int(v) for v in L]
    pos = _congruence(Q, [max(v, 0) for v in L])
    neg = _congruence(Q, [max(-v, 0) for v in L])
    den = 2 ** (42 + 2 * Q_BITS)
    return np.array([[Fraction(int(pos[i, j]) - int(neg[i, j]), den) for j in range(Q.shape[0])] for i in range(Q.shape[0])], dtype=object)


def exact_minv(Q, lam, rho, m):
    """Q diag(1 / (2 (lam + rho m))) Q' (every weight positive), rounded to double once."""
    S = 200
    W = []
    for v in lam:
        den = 2 * (Fraction(float(v)) + Fraction(float(rho)) * int(m))
        assert den > 0
        W.append(int(round(Fraction(2 ** S) / den)))
    T = _congruence(Q, W)
    den = 2 ** (S + 2 * Q_BITS)
    n = Q.shape[0]
    return np.array([[float(Fraction(int(T[i, j]), den)) for j in range(n)] for i in range(n)])


# ------------------------------------------------------------------ the trust-region problem in the eigenbasis
def _dec(v):
    return Decimal(float(v))      # (exact: a double is a dyadic rational)


def psi_at(d, gh, sigma):
    """psi(sigma) = sum_k gh_k^2 / (d_k + sigma)^2 at 80 digits; d, gh: Decimals; +inf where a term divides by zero."""
    total = Decimal(0)
    for dk, gk in zip(d, gh):
        if gk == 0:
            continue
        den = DEC.add(dk, sigma)
        if den == 0:
            return Decimal('Infinity')
        w = DEC.divide(gk, den)
        total = DEC.add(total, DEC.multiply(w, w))
    return total


def _root(d, gh, rho2, sigma_lo):
    """The sigma > sigma_lo with psi(sigma) == rho2, certified to a relative 1e-60."""
    rho = DEC.sqrt(rho2)
    live = [(dk, gk) for dk, gk in zip(d, gh) if gk != 0]
    s = max([sigma_lo] + [DEC.subtract(DEC.divide(abs(gk), rho), dk) for dk, gk in live])
    hi = DEC.divide(DEC.sqrt(sum((DEC.multiply(gk, gk) for _, gk in live), Decimal(0))), rho)

    def certified(s):
        eps = DEC.multiply(s, Decimal('1e-60'))
        return s > 0 and psi_at(d, gh, DEC.subtract(s, eps)) >= rho2 >= psi_at(d, gh, DEC.add(s, eps))

    for _ in range(200):          # Newton on 1 / sqrt(psi) - 1 / rho from the left of the root: monotone
        psi = T = Decimal(0)
        for dk, gk in live:
            den = DEC.add(dk, s)
            if den == 0:
                psi = None
                break
            w = DEC.divide(gk, den)
            w2 = DEC.multiply(w, w)
            psi, T = DEC.add(psi, w2), DEC.add(T, DEC.divide(w2, den))
        if psi is None:
            break
        step = DEC.multiply(DEC.divide(psi, T), DEC.divide(DEC.subtract(DEC.sqrt(psi), rho), rho))
        nxt = DEC.add(s, step)
        if abs(step) <= DEC.multiply(abs(nxt), Decimal('1e-75')):
            s = nxt
            break
        s = nxt
    if certified(s):
        return s
    lo = max(sigma_lo, Decimal(0))
    hi = DEC.multiply(max(hi, lo), Decimal(2)) + Decimal(1)
    for _ in range(400):          # plain bisection: psi decreases in sigma
        mid = DEC.divide(DEC.add(lo, hi), Decimal(2))
        if psi_at(d, gh, mid) > rho2:
            lo = mid
        else:
            hi = mid
    s = DEC.divide(DEC.add(lo, hi), Decimal(2))
    assert certified(s), 'no certified root'
    return s


_exact_cache = {}


def exact(lam, gh, rho2, eq):
    """min sum_k lam_k y_k^2 + 2 gh_k y_k  s.t. |y|^2 == rho2 (eq) or <= rho2: dict(value (Fraction), mu (Fraction), y (floats, by
    eigen-index; in the hard case WITHOUT the tau q_min part), tau2 (Fraction, hard case), branch (0 interior, 1 boundary, 2 hard
    case), sigma).  With <= and lambda_min == 0 the hard rule is asked, as the kernels document it: g without a component in the lowest
    eigenspace and psi_reg <= rho2 is branch 2 (mu = 0, any point of the lowest eigenspace may be added)."""
    key = (tuple(float(v) for v in lam), tuple(float(v) for v in gh), float(rho2), bool(eq))
    if key not in _exact_cache:
        _exact_cache[key] = _exact(*key)
    return _exact_cache[key]


def _exact(lam, gh, rho2, eq):
    L, G, R2 = [Fraction(v) for v in lam], [Fraction(v) for v in gh], Fraction(rho2)
    n = len(L)
    lmin = min(L)
    d = [v - lmin for v in L]
    if not eq and lmin > 0 and sum(g * g / (v * v) for g, v in zip(G, L)) <= R2:
        return dict(branch=0, mu=Fraction(0), value=sum(-g * g / v for g, v in zip(G, L)), y=np.array([float(-g / v) for g, v in zip(G, L)]),
                    tau2=Fraction(0), sigma=None)
    sigma_lo = lmin if (not eq and lmin > 0) else Fraction(0)
    if sigma_lo == 0 and all(g == 0 for g, dk in zip(G, d) if dk == 0):
        psi_reg = sum((g / dk) ** 2 for g, dk in zip(G, d) if dk != 0)
        if psi_reg <= R2:
            y = [(-g / dk if dk != 0 else Fraction(0)) for g, dk in zip(G, d)]
            tau2 = R2 - psi_reg
            value = sum(v * yk * yk + 2 * g * yk for v, g, yk in zip(L, G, y)) + lmin * tau2
            return dict(branch=2, mu=-lmin, value=value, y=np.array([float(v) for v in y]), tau2=tau2, sigma=Decimal(0))
    dd, gd = [_dec(float(v)) for v in d], [_dec(v) for v in gh]
    s = _root(dd, gd, _dec(rho2), _dec(float(sigma_lo)))
    y, value = [], Decimal(0)
    for k in range(n):
        yk = Decimal(0) if gd[k] == 0 else -DEC.divide(gd[k], DEC.add(dd[k], s))
        y.append(float(yk))
        value = DEC.add(value, DEC.add(DEC.multiply(_dec(lam[k]), DEC.multiply(yk, yk)), DEC.multiply(Decimal(2), DEC.multiply(gd[k], yk))))
    return dict(branch=1, mu=Fraction(s) - lmin, value=Fraction(value), y=np.array(y), tau2=Fraction(0), sigma=s)


def exact_case(c, relop):
    """exact() of a case, and the optimum of f0 itself: value + (h'P0 h - q0'h + r0), the constant of x = y - h."""
    e = exact(c['lam'], c['gh'], c['rho2'], relop == '==')
    hh = c['Q'].T.dot(c['h'])                                  # (exact: h is -1/2 or 0, Q dyadic)
    const = sum(Fraction(float(v)) * Fraction(float(t)) ** 2 for v, t in zip(c['lam'], hh)) \
        - sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(c['q0'], c['h'])) + Fraction(c['r0'])
    return e, e['value'] + const


def expected_branch(c, relop):
    """exact's branch; the 2^-47 member of the threshold pair is BELOW the kernels' threshold and is treated as the hard case."""
    return 2 if c['rhs'] == 'thr47' else exact_case(c, relop)[0]['branch']


def f_scale(c):
    """The scale of an error in the optimal value: |A|_F rho^2 + 2 |g| rho + |r0|."""
    rho = math.sqrt(c['rho2'])
    return float(np.linalg.norm(c['P0'])) * c['rho2'] + 2.0 * float(np.linalg.norm(c['g'])) * rho + abs(c['r0'])


def y_of(c, x):
    """y = s o x + beta / (2 s) of a point (s == 1 on this lattice)."""
    return np.asarray(x, dtype=np.float64) + c['h']


def norm(v):
    return math.sqrt(math.fsum(float(t) * float(t) for t in v))


def figures(c, relop, out):
    """(lam, f, feas) of one result (a dictionary with lam, bound, x, branch) against the exact reference, each relative to its
    scale: |A|_F, f_scale, rho.  feas is | |y| - rho | / rho on the boundary and the excess (|y| - rho) / rho, if any, inside."""
    e, opt = exact_case(c, relop)
    fro = float(np.linalg.norm(c['P0']))
    dlam = float(np.max(np.abs(np.asarray(out['lam']) - np.sort(c['lam'])))) / fro if fro else float(np.max(np.abs(out['lam'])))
    df = float(abs(Fraction(float(out['bound'])) - opt)) / f_scale(c)
    rho = math.sqrt(c['rho2'])
    ny = norm(y_of(c, out['x']))
    feas = abs(ny - rho) / rho if (relop == '==' or int(out['branch']) != 0) else max(ny - rho, 0.0) / rho
    return dlam, df, feas


def secular_stop_holds(c, mu):
    """The stop rule of the secular iteration, judged from the multiplier that a kernel reports (Tier A: lam and gh are exact).  The
    kernel holds sigma and reports mu = fl(sigma - lam_min): sigma is any number that rounds to that mu.  Over those sigma, either
      (a) | sqrt(psi(sigma)) - rho | <= 2^-49 rho   (SECULAR_RTOL = 2^-50 plus the rounding of a tree sum of up to 128 positive terms
                                                     and of its root, under 2^-50.7), or
      (b) psi - rho^2 changes sign within two floats of sigma   (the "step does not move sigma" stop).
    Where mu + lam_min is exact (lam_min == 0, or nothing lost in the subtraction) the set is the one point sigma = mu + lam_min."""
    lmin = float(np.min(c['lam']))
    mu = float(mu)
    lo = (Fraction(mu) + Fraction(float(np.nextafter(mu, -np.inf)))) / 2 + Fraction(lmin)
    hi = (Fraction(mu) + Fraction(float(np.nextafter(mu, np.inf)))) / 2 + Fraction(lmin)
    s0 = Fraction(mu) + Fraction(lmin)
    if lmin == 0.0 or (Fraction(float(s0)) == s0 and s0 != 0 and np.spacing(abs(float(s0))) >= np.spacing(abs(mu))):
        lo = hi = s0                                           # the one double that sigma can have been
    if hi <= 0:
        return False
    d = [_dec(v - lmin) for v in c['lam']]
    gd = [_dec(v) for v in c['gh']]
    rho2 = _dec(c['rho2'])
    as_dec = lambda f: DEC.divide(Decimal(f.numerator), Decimal(f.denominator))
    ulp = Fraction(float(np.spacing(max(float(hi), 5e-324))))
    tiny = Fraction(1, 2 ** 1100)
    psi_lo, psi_hi = psi_at(d, gd, as_dec(max(lo, tiny))), psi_at(d, gd, as_dec(hi))
    up, down = DEC.multiply(rho2, _dec((1.0 + 2.0 ** -49) ** 2)), DEC.multiply(rho2, _dec((1.0 - 2.0 ** -49) ** 2))
    a = psi_hi <= up and psi_lo >= down
    b = psi_at(d, gd, as_dec(max(lo - 2 * ulp, tiny))) >= rho2 >= psi_at(d, gd, as_dec(hi + 2 * ulp))
    return bool(a or b)


# ------------------------------------------------------------------ the setups
def setups(n):
    """[(tier, spectrum, Q, lam, P0)] of one size, m = n."""
    return [(tier, name) + v for (tier, name), v in matrices(n).items()]


def given_rho_batch(n):
    """Tier A, m = n: (P0s, lams) of four diagonal problems for the given-rho checks -- lambda_min = -2 with multiplicity n // 3, -1,
    -2 once (in the last coordinate: slot 1 of the last lane at n = 128), and 1."""
    k = np.arange(n)
    lams = [spectrum('multi', n), np.array([-1.0, 1.0, 2.0])[k % 3], np.where(k == n - 1, -2.0, 1.0 + k % 3), 1.0 + k % 3]
    return np.stack([np.diag(v) for v in lams]), lams


# ------------------------------------------------------------------ measured constants
# The worst figures of the NumPy restatements (spectral_batch_cases.restate for n <= 64, spectral_wide_cases.restate past it,
# admm_setup_cases.restate) against exact / exact_minv over the WHOLE lattice -- every size of SIZES + SIZES_WIDE, both relops, both
# tiers --, each rounded up.  They are never taken from a device.  tests/test_spectrum_lattice_cpu.py asserts that the restatements stay
# within them (every case up to n = 64, a fixed subset past it); tests/test_gpu_spectrum_lattice.py allows the kernels ten times each,
# the project's standing margin for fma and fixed-order sums against NumPy's.
LAM_MEASURED = 6.0e-16       # measured 5.96e-16 |A|_F     (n = 64, Tier B, 'multi'); 2.4e-16 past n = 64
F_MEASURED = 6.8e-15         # measured 6.76e-15 f_scale   (n = 64, Tier B, 'pm', g = 0: |q_min| drifts from 1 over 18 sweeps); 2.3e-16 past n = 64
FEAS_MEASURED = 1.8e-14      # measured 1.75e-14 rho       (n = 64, Tier B, 'pm', one component); 7.9e-16 past n = 64
MINV_MEASURED = 4.4e-14      # measured 4.37e-14 max|Minv| (n = 63, Tier B, 'two'); 2.4e-15 past n = 64
# (lambda_min of the setups: 2.0e-16 |P0|_F at worst, inside admm_setup_cases.LMIN_MEASURED = 7.8e-16, whose bound the GPU test keeps)
# Two independent methods on the generic right-hand sides: spectral_batch_cases.independent (LAPACK's eigh and a bracketed root at
# 8.9e-16) against exact.  eigh is backward stable to a small multiple of n eps |A|_F, 1.4e-14 at n = 128, and the value moves by
# rho^2 times that; 1e-12 of f_scale leaves that estimate a factor of 70.
INDEPENDENT_RTOL = 1e-12
