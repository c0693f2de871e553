"""The case lattice of the one-variable solver (csrc/onevar.h, csrc/cd_phase1_sep.h): degenerate one-variable quadratics by
construction, shared by tests/test_onevar_lattice_cpu.py (oracle against the reference's golden g12, host build of every variant
against the oracle) and tests/test_gpu_onevar_lattice.py (the same variants on the device).  Deterministic: fixed seeds, nothing
read from a clock.

ONEVAR LATTICE (`onevar_lattice()`): cases (objective, list of 1..4 constraint atoms, slack), stored as indices into the tables
OBJECTIVES / ATOMS / SLACKS.

  atoms       sc (x - a)(x - b) <= 0 for a <= b in PTS = {-2, -1, -1/2, 0, 1/2, 1, 2} and sc in {1, -1, 1/4} (a == b: zero
              discriminant; end points are dyadic, so equal end points of different constraints are EQUAL doubles); the linear pairs
              x <= a, -x <= -a; the equalities (x - a)^2 - 1/4 == 0 and +-(x^2 - 1) == 0; atoms with |p| or |q| at the 1e-4
              threshold of get_feasible_intervals (1e-4 itself: linear / constant by the threshold, its upper neighbour and 1.5e-4:
              quadratic / linear, 5e-5: below), among them SURVEY.md A.7's "always feasible" (5e-5, 5e-5, 10); constants
              (p = q = 0) with r of either sign.
  lists       built by construction (`_lists`): a disc (or the ray x <= 2) with 1, 2, 3 disjoint holes -> sets of 2, 3, 4 pieces
              (PTS has five points strictly inside [-2, 2], so three holes inside the disc touch its rim at slack 0: the fourth piece
              is then a single point, which the sweep drops, and exists at the positive slacks; under the ray all four are there at
              slack 0); pairs that touch in one point; identical pairs (also the same interval at two scales); nested pairs and pairs
              sharing one end; the whole line; one-sided rays; each also padded to greater lengths with constraints that hold
              everywhere.  Random lists of 1..4 atoms are added to them (they alone give 45 % None and next to no set of three pieces).
  objectives  vertex inside / outside / on an end point of a piece; p0 < 0 about 0 and about +-1/2, so that end points placed
              symmetrically tie exactly; p0 = 0 with q0 != 0; p0 = q0 = 0.  Sets with an infinite end come from the ray lists.
  slacks      {0, 1e-4, 1/4, 3/4, -1e-5}.

  Status -2 (the reference's NameError, OneVarQuadraticFunction.eval at +-inf with P = q = 0) cannot be reached through onevar_qcqp:
  an objective with p0 = q0 = 0 takes the uniform-draw branch (utilities.py:266-267) before any end point is evaluated.  The CPU
  test asserts that the oracle never returns it on the lattice, instead of a cell of 30.

VISIT LATTICE (`visit_lattice()`): phase-1 coordinate visits (constraint list, x_i before the visit).
  band class  one constraint p x^2 + r == 0: p in {1, 1/4, 4, 2e-4, nextafter(1e-4)}, r in {-1, -1/4, -4, -1e-3 and both
              neighbours' side (-2e-3, nextafter(-1e-3, -1)), 0, 1/2, -1e-5}; x_i generic and targeted: |f(x_i)| = v for v = 0,
              viol_tol (the bisection never starts: viol - viol_tol <= 0), viol_tol + tol k for k = 1, 3, 7, 15 (viol - viol_tol within
              a few ulps of k tol: the k-th-from-last midpoint (ss + es) / 2 falls within the band visits' `guard` of 0), and large.
  mixed       lists of 1..4 atoms; the first is bounded in 85 % of the cases (the set stays bounded: the visit draws a point), the rest
              end in the unbounded-set status.
  Constraints with p = q = 0 are excluded here, and only here: the reference filters them out before the visit (qcqp.py:115-116
  keeps f.P != 0 or f.q != 0) and qcqpmi_finalize never attaches one to a coordinate, so p1_sep_visit_core is never handed one.

FAMILIES (`family()`, FAMILY_RUNS, FAMILY_BATCH): separable problems whose coordinates carry lists from the lattice with a bounded, non-empty feasible set at
slack 0, for whole coordinate-descent runs through the real kernels.
"""
import ctypes
import itertools
import zlib

import numpy as np

PTS = [-2., -1., -.5, 0., .5, 1., 2.]
SLACKS = [0., 1e-4, .25, .75, -1e-5]
RELCODE = {'<=': 1, '==': 2}
RELSTR = {1: '<=', 2: '=='}
EPS_UP = float(np.nextafter(1e-4, 1.0))
A7 = (5e-5, 5e-5, 10., '<=')

OBJECTIVES = [
    (1., 0., 0.), (1., -1., 0.), (1., -4., 0.), (1., -6., 0.), (1., 3., 0.), (2., 1., 0.), (1., 2., -1.),      # vertex 0, 1/2, 2, 3, -3/2, -1/4, -1
    (-1., 0., 0.), (-1., 1., 0.), (-1., -1., 0.), (-.25, 0., 1.), (-1., .5, 2.),                               # concave: about 0, 1/2, -1/2, 0, 1/4
    (0., 1., 0.), (0., -1., 0.), (0., 2., 1.),                                                                # linear
    (0., 0., 0.), (0., 0., 3.),                                                                               # zero: a uniform draw
]
ZERO_OBJ = [k for k, o in enumerate(OBJECTIVES) if o[0] == 0. and o[1] == 0.]
CONCAVE_OBJ = [k for k, o in enumerate(OBJECTIVES) if o[0] < 0.]


def _atoms():
    A = []
    for a, b in itertools.combinations_with_replacement(PTS, 2):
        for sc in (1., -1., .25):
            A.append((sc, -sc * (a + b), sc * a * b, '<='))
    for a in PTS:
        A.append((0., 1., -a, '<='))
        A.append((0., -1., a, '<='))
    for a in PTS:
        A.append((1., -2. * a, a * a - .25, '=='))
    A += [(1., 0., -1., '=='), (-1., 0., 1., '==')]
    for t in (1e-4, EPS_UP, 5e-5, 1.5e-4):
        A += [(t, 0., -1., '<='), (-t, 1., 0., '<='), (0., t, -1., '<='), (0., -t, -1., '<='), (t, 0., -1., '==')]
    A += [A7, (0., 0., 1., '<='), (0., 0., -1., '<='), (0., 0., 1e-5, '=='), (0., 0., -.5, '=='), (1., 0., 1., '<=')]
    return A


ATOMS = _atoms()
_IDX = {}
for _k, _a in enumerate(ATOMS):
    _IDX.setdefault(_a, _k)


def quad(sc, a, b):
    return _IDX[(sc, -sc * (a + b), sc * a * b, '<=')]


def le(a):
    return _IDX[(0., 1., -a, '<=')]


def ge(a):
    return _IDX[(0., -1., a, '<=')]


def eqs(a):
    return _IDX[(1., -2. * a, a * a - .25, '==')]


EQ1 = _IDX[(1., 0., -1., '==')]
EQ1N = _IDX[(-1., 0., 1., '==')]
ALWAYS = [_IDX[(0., 0., -1., '<=')], _IDX[A7], quad(-1., 0., 0.), _IDX[(1e-4, 0., -1., '<=')], quad(-1., 1., 1.)]
# (these hold everywhere; 1e-4 x^2 - 1 <= 0 does because 1e-4 is not above the threshold: the atom is read as a constant)
IS_CONST = np.array([a[0] == 0. and a[1] == 0. for a in ATOMS])
IS_BOUNDED = np.array([(a[3] == '<=' and a[0] > 1e-3) or (a[3] == '==' and abs(a[0]) > 1e-3) for a in ATOMS])


def _lists():
    """The constructed constraint lists, each (atom indices, tag); tag 's' = symmetric about 0 or 1/2 (concave objectives tie),
    'u' = the set has an infinite end."""
    L = []
    hole = lambda a, b: quad(-1., a, b)
    hole_sets = [[(-1., -.5)], [(0., .5)], [(-.5, .5)], [(-1., 1.)], [(.5, 1.)], [(0., 0.)],
                 [(-1., -.5), (0., .5)], [(-1., 0.), (.5, 1.)], [(-1., -.5), (.5, 1.)], [(-1., -.5), (1., 2.)], [(-2., -1.), (1., 2.)],
                 [(-2., -1.), (-.5, 0.), (.5, 1.)], [(-1., -.5), (0., .5), (1., 2.)], [(-2., -1.), (0., .5), (1., 2.)],
                 [(-2., -1.), (-.5, 0.), (1., 2.)], [(-1., -.5), (0., .5), (1., 1.)], [(-2., -1.), (-.5, .5), (1., 2.)]]
    for hs in hole_sets:
        sym = sorted(hs) == sorted((-b, -a) for a, b in hs)
        for outer, tag in ((quad(1., -2., 2.), ''), (quad(.25, -2., 2.), ''), (le(2.), 'u'), (ge(-2.), 'u')):
            L.append(([outer] + [hole(*h) for h in hs], ('s' if sym and tag == '' else '') + tag))
    tri = [t for t in itertools.combinations(PTS, 3)]
    for a, b, c in tri[::2]:                                       # [a, b] and [b, c] touch in b
        L.append(([quad(1., a, b), quad(1., b, c)], ''))
        L.append(([quad(.25, a, b), quad(1., b, c), ge(a)], ''))
    for a, b in itertools.combinations(PTS, 2):
        L.append(([quad(1., a, b), ge(b)], ''))                    # one point, by a linear bound
        L.append(([le(b), ge(b)], ''))                             # equal linear bounds
        L.append(([quad(1., a, b), quad(1., a, b)], 's' if a + b in (0., 1., -1.) else ''))      # identical
        L.append(([quad(1., a, b), quad(.25, a, b)], 's' if a + b in (0., 1., -1.) else ''))     # the same interval at two scales
        L.append(([quad(1., a, b), le(b), ge(a)], 's' if a + b in (0., 1., -1.) else ''))
        L.append(([quad(-1., a, b), quad(-1., a, b)], 'u'))
        L.append(([quad(1., a, b)], 's' if a + b in (0., 1., -1.) else ''))
        L.append(([quad(-1., a, b)], 'u'))
        L.append(([le(a), le(b)], 'u'))
        L.append(([ge(a), quad(-1., a, b)], 'u'))
        L.append(([le(b), quad(-1., a, b)], 'u'))
    for a, b, c, d in itertools.combinations(PTS, 4):
        if (a, b, c, d)[0] + d == 0. or len(L) % 2:
            L.append(([quad(1., a, d), quad(1., b, c)], 's' if a + d == 0. and b + c == 0. else ''))      # nested
        L.append(([quad(1., a, c), quad(1., a, d)], ''))                                                   # sharing the left end
        L.append(([quad(1., a, c), quad(.25, b, d)], ''))                                                  # overlapping
    for a in PTS:
        L.append(([eqs(a)], 's' if a in (0., .5, -.5) else ''))
        L.append(([eqs(a), quad(1., -2., 2.)], ''))
        L.append(([eqs(a), le(a)], ''))
        L.append(([le(a)], 'u'))
        L.append(([ge(a)], 'u'))
        L.append(([quad(1., a, a)], ''))                            # zero discriminant: the point a
        L.append(([quad(-1., a, a)], 'u'))                          # two rays that touch in a: the whole line
        L.append(([quad(.25, a, a), quad(-1., a, a)], ''))
    # three events on one key: a zero-width piece of an equality (+1, -1) under the end of an interval, and three intervals that
    # meet in one point
    for a in PTS:
        for e in (a - .5, a + .5):
            for lo in PTS:
                if e in PTS and lo < e and (int(2 * (a + lo)) % 2 == 0):
                    L.append(([eqs(a), quad(1., lo, e)], ''))
                    L.append(([quad(.25, lo, e), eqs(a)], ''))
    for a, b, c in tri[1::2]:
        L.append(([quad(1., a, b), quad(1., b, c), quad(.25, -2., b) if a > -2. else quad(.25, a, b)], ''))
        L.append(([quad(1., a, c), le(b), quad(1., a, b)], ''))
    L += [([EQ1], 's'), ([EQ1N], 's'), ([EQ1, EQ1N], 's'), ([EQ1, quad(1., -2., 2.)], 's'), ([EQ1, le(1.)], ''), ([EQ1, ge(1.)], 'u'),
          ([EQ1, eqs(.5)], ''), ([EQ1, eqs(-.5), quad(1., -2., 2.)], ''), ([eqs(-.5), eqs(.5)], 's'), ([eqs(0.), EQ1], 's')]
    for k in ALWAYS:
        L.append(([k], 'u'))
        L.append(([k, k], 'u'))
    for k, a in enumerate(ATOMS):
        if abs(a[0]) in (1e-4, EPS_UP, 5e-5, 1.5e-4) or (a[0] == 0. and abs(a[1]) in (1e-4, EPS_UP, 5e-5, 1.5e-4)) or IS_CONST[k]:
            L.append(([k], 'u'))
            L.append(([k, quad(1., -2., 2.)], 's'))
            L.append(([quad(1., -1., 1.), k, le(.5)], ''))
    # the same lists padded with constraints that hold everywhere, up to length 4
    out = list(L)
    for j, (l, tag) in enumerate(L):
        for extra in (1, 2, 3):
            if len(l) + extra <= 4 and (j + extra) % 3 != 0:
                pad = [ALWAYS[(j + e) % len(ALWAYS)] for e in range(extra)]
                out.append((l + pad if j % 2 else pad + l, tag))
    return out


_CACHE = {}


def onevar_lattice():
    """dict(obj (N,) int16, atom (N, 4) int16 with -1 padding, nf (N,), slack (N,) int16) of the lattice."""
    if 'onevar' in _CACHE:
        return _CACHE['onevar']
    rs = np.random.RandomState(20240611)
    rows = []
    nobj = len(OBJECTIVES)
    for j, (l, tag) in enumerate(_lists()):
        for si in range(len(SLACKS)):
            if (j + si) % 5 in (1, 3) and si not in (0, 1):       # thin the wide slacks
                continue
            objs = set(int(o) for o in rs.choice(nobj, size=2, replace=False))
            if (j + si) % 3 == 0:
                objs.add(ZERO_OBJ[(j + si) % len(ZERO_OBJ)])
            if 's' in tag:
                objs.add(CONCAVE_OBJ[(j + si) % 3])                # about 0, 1/2, -1/2 in turn
                if len(l) == 1:
                    objs.update(CONCAVE_OBJ[:4])
            if 'u' in tag and (j + si) % 2:
                objs.add(ZERO_OBJ[j % len(ZERO_OBJ)])
            for o in sorted(objs):
                rows.append((o, l, si))
    for k in (1, 2, 3, 4):
        for t in range(350):
            l = [int(a) for a in rs.randint(0, len(ATOMS), size=k)]
            rows.append((int(rs.randint(nobj)), l, int(rs.choice([0, 0, 1, 2, 3, 4]))))
    N = len(rows)
    obj = np.array([r[0] for r in rows], dtype=np.int16)
    atom = np.full((N, 4), -1, dtype=np.int16)
    nf = np.zeros(N, dtype=np.int32)
    for i, r in enumerate(rows):
        nf[i] = len(r[1])
        atom[i, :nf[i]] = r[1]
    slack = np.array([r[2] for r in rows], dtype=np.int16)
    _CACHE['onevar'] = dict(obj=obj, atom=atom, nf=nf, slack=slack)
    return _CACHE['onevar']


def atom_rows(idx):
    """(len(idx), 4) array of (p, q, r, relop code)."""
    return np.array([[ATOMS[k][0], ATOMS[k][1], ATOMS[k][2], RELCODE[ATOMS[k][3]]] for k in idx], dtype=np.float64).reshape(-1, 4)


def onevar_arrays(lat=None):
    """The lattice in the layout of qcqpmi_onevar_qcqp_batch: f0 (N, 3), fs (N, 4, 4) (unused slots zero), nf int32, s (N,)."""
    lat = lat or onevar_lattice()
    N = len(lat['obj'])
    table = atom_rows(range(len(ATOMS)))
    f0 = np.array(OBJECTIVES, dtype=np.float64)[lat['obj']]
    fs = np.zeros((N, 4, 4))
    used = lat['atom'] >= 0
    fs[used] = table[lat['atom'][used]]
    s = np.array(SLACKS)[lat['slack']]
    return np.ascontiguousarray(f0), np.ascontiguousarray(fs), np.ascontiguousarray(lat['nf'].astype(np.int32)), np.ascontiguousarray(s)


def checksum(*arrays):
    """(total length, crc32) of the arrays' bytes."""
    c, n = 0, 0
    for a in arrays:
        b = np.ascontiguousarray(a).tobytes()
        c = zlib.crc32(b, c)
        n += len(b)
    return n, c & 0xffffffff


# ---------------------------------------------------------------- the visit lattice
BAND_P = [1., .25, 4., 2e-4, EPS_UP]
BAND_R = [-1., -.25, -4., -1e-3, -2e-3, float(np.nextafter(-1e-3, -1.)), 0., .5, -1e-5]
TOL, VIOL_TOL = 1e-4, 1e-2


def visit_lattice():
    """dict(cons (N, 4, 4), nf int32, xi (N,), nband): the first nband cases are the band class, ordered so that runs of one
    (p, r) have odd length (the fused variants then meet pairs and padding in both positions)."""
    if 'visit' in _CACHE:
        return _CACHE['visit']
    cases = []
    generic = [0., 1., -1., 1. + 1e-3, -(1. - 1e-3), 1. + 4e-3, 1. - 6e-3, 1.1, .9, 3., -1e3, 1e-8, .5, 2., -2., 0.7071067811865476]
    for p in BAND_P:
        for r in BAND_R:
            xs = list(generic)
            for k, v in enumerate([0., VIOL_TOL, VIOL_TOL + 1e-12, VIOL_TOL + TOL, VIOL_TOL + 3 * TOL, VIOL_TOL + 7 * TOL, VIOL_TOL + 15 * TOL,
                                   float(np.nextafter(VIOL_TOL + TOL, 1.)), float(np.nextafter(VIOL_TOL + TOL, 0.)), .5]):
                if v - r >= 0.:
                    x = float(np.sqrt((v - r) / p))
                    xs.append(-x if k % 2 else x)
                if -v - r > 0.:                                     # f(x) = -v: inside the band
                    xs.append(float(np.sqrt((-v - r) / p)))
            if len(xs) % 2 == 0:
                xs.append(.25)
            for x in xs:
                cases.append(([(p, 0., r, '==')], x))
    nband = len(cases)
    bounded = [k for k in range(len(ATOMS)) if IS_BOUNDED[k]]
    allowed = [k for k in range(len(ATOMS)) if not IS_CONST[k]]
    others = [k for k in allowed if not IS_BOUNDED[k]]
    rs = np.random.RandomState(1)
    xs = PTS + [3., .3, -.7, 1.004, 1.02, -1.5, 2.5]
    for k in (1, 2, 3, 4):
        for t in range(600):
            first = bounded[rs.randint(len(bounded))] if rs.rand() < .85 else others[rs.randint(len(others))]
            l = [first] + [allowed[j] for j in rs.randint(0, len(allowed), size=k - 1)]
            cases.append(([ATOMS[a] for a in l], float(xs[rs.randint(len(xs))])))
    N = len(cases)
    cons = np.zeros((N, 4, 4))
    nf = np.zeros(N, dtype=np.int32)
    for i, (l, _) in enumerate(cases):
        nf[i] = len(l)
        for j, a in enumerate(l):
            cons[i, j] = [a[0], a[1], a[2], RELCODE[a[3]]]
    _CACHE['visit'] = dict(cons=cons, nf=nf, xi=np.array([c[1] for c in cases]), nband=nband)
    return _CACHE['visit']


ONEVAR_VARIANTS = {'sweep4': 0, 'sweep2': 1, 'sweep1': 2, 'single4': 3, 'single2': 4, 'single1': 5}
ONEVAR_MAXC = {'sweep4': 4, 'sweep2': 2, 'sweep1': 1, 'single4': 4, 'single2': 2, 'single1': 1}
VISIT_VARIANTS = {'core1': 0, 'core4': 1, 'band': 2, 'band_n2': 3, 'band_n2_fasta': 4}


def onevar_subset(name, nf):
    """Indices of the cases inside the contract of an onevar variant."""
    if name.startswith('single'):
        return np.nonzero(nf == 1)[0]
    return np.nonzero(nf <= ONEVAR_MAXC[name])[0]


def visit_subset(name, vl):
    cons, nf = vl['cons'], vl['nf']
    band = (nf == 1) & (cons[:, 0, 1] == 0.) & (cons[:, 0, 3] == 2) & (cons[:, 0, 0] > 1e-4)
    if name == 'core1':
        return np.nonzero(nf == 1)[0]
    if name == 'core4':
        return np.arange(len(nf))
    if name == 'band':
        return np.nonzero(band)[0]
    return np.nonzero(band & (cons[:, 0, 2] < -1e-3))[0]


# ---------------------------------------------------------------- the oracle's answers
def oracle_onevar(orc, f0, fs, nf, s, mode, seed=0):
    """The oracle's onevar_qcqp on every case: status (1 point, 0 None, < 0 raise), x (NaN unless status 1), nC, C (N, 5, 2) with
    NaN in the unused slots, draws.  mode = orc.RNG_KEYED: the draw key is (seed; restart = case; 0, 0, 0), the unit operators';
    orc.RNG_MT: numpy's global stream seeded with the case index, as the golden g12 was recorded."""
    L = orc.lib()
    N = len(nf)
    st = np.zeros(N, dtype=np.int32)
    x = np.full(N, np.nan)
    nC = np.zeros(N, dtype=np.int32)
    Cs = np.full((N, 5, 2), np.nan)
    draws = np.zeros(N, dtype=np.int64)
    dp = ctypes.POINTER(ctypes.c_double)
    rng = orc.Rng(orc.RNG_KEYED, seed) if mode == orc.RNG_KEYED else None
    cap = 18
    Cout = np.zeros(2 * cap)
    ncv = np.zeros(1, dtype=np.int64)
    for i in range(N):
        mf = int(nf[i])
        fs3 = np.ascontiguousarray(fs[i, :max(mf, 1), :3]).ravel()
        rel = (ctypes.c_int * max(mf, 1))(*[int(v) for v in fs[i, :mf, 3]])
        if mode == orc.RNG_KEYED:
            rng.set_restart(i)
            rng.set_ctx(0, 0, 0)
        else:
            np.random.seed(i)
            rng = orc.Rng(orc.RNG_MT, 0, from_numpy_global=True)
        d0 = rng.draws
        xv = ctypes.c_double(0.)
        got = L.orc_onevar_qcqp(f0[i, 0], f0[i, 1], f0[i, 2], fs3.ctypes.data_as(dp), rel, mf, float(s[i]), rng.h, ctypes.byref(xv),
                                Cout.ctypes.data_as(dp), cap, ncv.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        st[i] = got
        draws[i] = rng.draws - d0
        if got == 1:
            x[i] = xv.value
        nC[i] = ncv[0]
        assert ncv[0] <= 5
        Cs[i, :ncv[0]] = Cout[:2 * ncv[0]].reshape(-1, 2)
    return dict(status=st, x=x, nC=nC, C=Cs, draws=draws)


def oracle_visits(orc, cons, nf, xi, seed, sweep, tol=TOL, viol_tol=VIOL_TOL):
    """The oracle's phase-1 visit of every case, each as a problem of ONE coordinate (keyed draws: restart = case, coordinate 0):
    x after the visit, status (0 or the code of the raise), moved (the value changed), vafter (the oracle's max violation at the
    returned point: its evaluation (p x + q) x + r is the visit's own).  Where the reference raises: _steps_before_the_raise."""
    import scipy.sparse as sp
    N = len(nf)
    xo = np.array(xi, dtype=np.float64).copy()
    st = np.zeros(N, dtype=np.int32)
    moved = np.zeros(N, dtype=np.int32)
    va = np.zeros(N)
    L = orc.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    rng = orc.Rng(orc.RNG_KEYED, seed)
    zero = (sp.csr_matrix((1, 1)), np.zeros(1), 0., None)
    for i in range(N):
        funcs = [zero] + [(sp.csr_matrix(np.array([[c[0]]])), np.array([c[1]]), float(c[2]), RELSTR[int(c[3])]) for c in cons[i, :nf[i]]]
        prob = orc.Problem(funcs)
        rng.set_restart(i)
        x = np.array([xi[i]])
        st[i] = L.orc_cd_visits(prob.h, x.ctypes.data_as(dp), 1, int(sweep), 0, 1, 0., viol_tol, tol, rng.h)
        xo[i] = x[0]
        moved[i] = xo[i] != xi[i]
        if st[i] < 0:
            xo[i], moved[i] = _steps_before_the_raise(orc, rng, cons[i, :nf[i]], float(xi[i]), int(sweep), tol, viol_tol)
            x[0] = xo[i]
        va[i] = prob.max_violation(x)
    return dict(x=xo, status=st, moved=moved, vafter=va)


def _steps_before_the_raise(orc, rng, cons, xi, sweep, tol, viol_tol):
    """A visit on which the reference raises (np.random.uniform on an unbounded piece, at some slack of the bisection): the
    exception ends the reference's whole run, so it defines no x_i.  The engine reports the status and keeps what the steps
    BEFORE the raise did, by the reference's own loop (qcqp.py:122-131) replayed here on the oracle's onevar_qcqp with the visit's
    draw keys: a step that succeeded lowers the achieved slack (the visit counts as moved); its point is taken at once where the
    set has an infinite end (the draw landed in a bounded piece), and only at the end of the bisection -- never reached -- where
    the set is bounded.  Returns (x_i the engine leaves, moved)."""
    fs = [(c[0], c[1], c[2], RELSTR[int(c[3])]) for c in cons]
    viol = max((abs(f) if c[3] == 2 else max(f, 0.)) for c, f in ((c, xi * (c[0] * xi + c[1]) + c[2]) for c in cons))
    ss, es, it, x, moved = -tol, viol - viol_tol, 0, xi, 0
    while es - ss > tol:
        s = (ss + es) / 2.
        rng.set_ctx(0, sweep, it)
        it += 1
        try:
            xn, Cs = orc.onevar_qcqp((0., 0., 0.), fs, s, rng)
        except RuntimeError:
            return x, moved
        if xn is None:
            ss = s
        else:
            es, moved = s, 1
            if any(np.isinf(v) for piece in Cs for v in piece):
                x = xn
    raise AssertionError('the replay of a raising visit did not raise')


# ---------------------------------------------------------------- the comparison, shared by the host and the device tests
def _same(a, b):
    """== on doubles, NaN equal to NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def compare_onevar(got, ref, idx, maxc):
    """Cases (positions in idx) where a variant's answer differs from the oracle's in status, point, piece count or any piece.
    got: status, x, nC, C (len(idx), 5, 2) of the variant; ref: oracle_onevar over the whole lattice.  Equality is == on doubles;
    a slot past the piece count holds 0.0 where the variant has the slot and NaN where it has not."""
    st, x, nC, Cs = ref['status'][idx], ref['x'][idx], ref['nC'][idx], ref['C'][idx]
    bad = (got['status'] != st) | (got['nC'] != nC)
    bad |= ~_same(np.where(got['status'] == 1, got['x'], np.nan), x)
    bad |= (got['status'] != 1) & ~np.isnan(got['x'])
    for j in range(5):
        live = j < nC
        want = np.where(live[:, None], Cs[:, j], np.nan if j > maxc else 0.)
        bad |= ~(_same(got['C'][:, j, 0], want[:, 0]) & _same(got['C'][:, j, 1], want[:, 1]))
    return np.nonzero(bad)[0]


def compare_visits(got, ref, idx):
    """Cases where a visit variant differs from the oracle's visit in any of status, x after the visit, moved, vafter (== on
    doubles).  Where the reference raises, x / moved / vafter are those of the steps before the raise (oracle_visits)."""
    bad = (got['status'] != ref['status'][idx]) | ~_same(got['x'], ref['x'][idx]) | (got['moved'] != ref['moved'][idx]) | \
        ~_same(got['vafter'], ref['vafter'][idx])
    return np.nonzero(bad)[0]


def describe_onevar(i, f0, fs, nf, s):
    return 'case %d: f0 = %r, fs = %r, s = %r' % (i, tuple(f0[i]), [tuple(c) for c in fs[i, :nf[i]]], float(s[i]))


# ---------------------------------------------------------------- degenerate coordinate lists for whole runs
def _kind_lists(delta=.05, lin=.5):
    """The constraint list of each coordinate kind, as (p, q, r, relop): bounded and non-empty at slack 0 (a single point counts:
    phase 1 reaches it within viol_tol, phase 2 works at the slack it starts with)."""
    return {
        'touch': [(1., 1., -delta, '<='), (1., -1., -delta, '<=')],              # [-1, 0] and [0, 1], widened by r to [-eps, eps]
        'eq1_pair': [(1., 0., -1., '<='), (-1., 0., 1., '<=')],                  # x^2 == 1 as two inequalities
        'lin_eq': [(0., 1., -lin, '<='), (0., -1., lin, '<=')],                  # equal linear bounds
        'eq_shift': [(1., -1., 0., '==')],                                       # (x - 1/2)^2 == 1/4: an equality with a linear term
        'thr_lin': [(1e-4, 1., -1., '<='), (0., -1., -1., '<=')],                # 1e-4: read as linear (x <= 1), with x >= -1
        'thr_quad': [(1.5e-4, 1., -1., '<='), (0., -1., -2., '<=')],             # 1.5e-4: quadratic, roots 0.99985.. and -6667.6..
        'holes2': [ATOMS[quad(1., -2., 2.)], ATOMS[quad(-1., -1., -.5)], ATOMS[quad(-1., .5, 1.)]],      # a disc with two holes
    }


def _objective(kind, n, seed=4):
    from qcqp_amd import problems
    if kind == 'ridge':            # least squares + ridge
        return problems.box_least_squares(n, max(4, n // 2), bound=1.0, seed=seed)[0][0]
    return problems.box_qp(n, seed=seed, zero_every=1)[0][0]       # 'zdiag': a zero diagonal


def family(name, n, objective='ridge', seed=4):
    """[(P, q, r, relop)] with the objective first.  mix7: the seven kinds of _kind_lists in turn (7 classes, up to 3 constraints
    per coordinate); mix23: the same with 23 widths of the touching pair and 23 values of the equal bounds (more classes than the
    class table of cd_phase2_kernel holds); one4: ONE constraint per coordinate, 4 classes -- the shifted equality, x^2 == 1, a
    disc, the 1.5e-4 atom (a quadratic just past the threshold: its feasible interval is about [-6667.7, 0.99985])."""
    import scipy.sparse as sp
    kinds = sorted(_kind_lists())
    funcs = [_objective(objective, n, seed)]
    for i in range(n):
        if name == 'one4':
            l = [[(1., -1., 0., '==')], [(1., 0., -1., '==')], [(.25, 0., -1., '<=')], [(1.5e-4, 1., -1., '<=')]][i % 4]
        else:
            j = i % 23 if name == 'mix23' else 0
            l = _kind_lists(delta=.05 + j / 230., lin=.5 - j / 46.)[kinds[i % len(kinds)]]
        for p, q, r, relop in l:
            qv = np.zeros(n)
            qv[i] = q
            funcs.append((sp.csr_matrix(([p], ([i], [i])), shape=(n, n)), qv, r, relop))
    return funcs


FAMILY_RUNS = [        # (tag, family, objective, n): Engine.cd_run, R = 21 restarts, first_index 3, num_iters 40
    ('mix7-ridge-48', 'mix7', 'ridge', 48), ('mix7-ridge-96', 'mix7', 'ridge', 96), ('mix7-zdiag-48', 'mix7', 'zdiag', 48),
    ('mix23-ridge-48', 'mix23', 'ridge', 48), ('mix23-zdiag-96', 'mix23', 'zdiag', 96),
    ('one4-ridge-48', 'one4', 'ridge', 48), ('one4-zdiag-96', 'one4', 'zdiag', 96),
]
FAMILY_R, FAMILY_FIRST, FAMILY_ITERS = 21, 3, 40
FAMILY_BATCH = [       # (tag, family, n): Engine.cd_batch_run, B = 3 objectives (ridge, ridge, zero diagonal), R = 8
    ('mix7-48', 'mix7', 48), ('mix7-112', 'mix7', 112), ('mix23-48', 'mix23', 48), ('one4-112', 'one4', 112),
]
BATCH_R, BATCH_FIRST = 8, 5


def batch_family(name, n):
    return [family(name, n, 'ridge', 4), family(name, n, 'ridge', 5), family(name, n, 'zdiag', 3)]


GENK, LINK = 3, 4       # L2_KIND_GENK / L2_KIND_LINK (csrc/cd_life_plan.h)
FAMILY_STREAM = [      # (tag, objective, n, (nmw, cs, kind) of the launch): Engine.cd_stream_run on the one4 family, one population
    ('one4-ridge-48', 'ridge', 48, (3, 0, GENK)), ('one4-zdiag-96', 'zdiag', 96, (3, 2, LINK)),
    ('one4-ridge-112', 'ridge', 112, (3, 2, GENK)), ('one4-zdiag-48', 'zdiag', 48, (3, 0, LINK)),
]


def stream_geometry(s):
    """(nmw, cs, kind) cd_life2_config (csrc/cd_life_plan.h) chooses for a separable problem of shape s (test_gpu_cd_run_domain.shape)
    with several classes or two constraints per coordinate and NB <= 64, or None where it refuses the problem."""
    NB = s['NB']
    if not (1 <= s['maxc'] <= 2 and 1 <= s['Kreal'] <= 4) or s['objclass'] not in (1, 2) or NB < 3:
        return None
    assert (s['maxc'] > 1 or s['Kreal'] > 1) and NB <= 64
    return 3, (0 if NB <= 4 else 2 if NB < 8 else 4), (LINK if s['objclass'] == 2 else GENK)
