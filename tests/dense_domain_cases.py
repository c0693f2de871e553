"""What tests/test_dense_domain_cpu.py and tests/test_gpu_dense_domain.py share: the families of the coupled-constraint
(dense) coordinate-descent path, the geometry table of dense_chain_mw_kernel as read from mw_geometry (csrc/cd_dense_mw.h), the
teacher-forced walker along the oracle's trajectories with its yardstick (the oracle against itself under a few ulps), and the
hand-built problems that fill the gap list (DN_GC = 64) and the segment list (DN_SC = 32) of csrc/cd_dense.h.  A plain
module, not a conftest: the test files import what they use."""
import ctypes as C
from collections import namedtuple

import numpy as np

DENSE_PATH = 32 << 4         # qcqpmi_debug_profile switch: take the dense path on small problems too (default: n > 64)
N_FORCED, N_DEFAULT = 40, 72  # three blocks, the last one of 8 coordinates / five blocks through the default dispatch
SEED, FIRST = 13, 5          # keyed stream of every walk
VISIT_TOL, BLOCK_TOL = 1e-8, 1e-6

# A: one m per class and boundary of mw_geometry
A_GRID = (1, 2, 63, 64, 65, 448, 449, 511, 512, 600, 896, 897, 1344, 1345, 1792, 1793, 2240, 2241, 2688, 2689, 3136, 3137, 3584)
A_R = 8
A_EXTRA = (600, 40, (15, 16, 17, 39))      # (m, R, compared restarts): another K-split and tile count
# m -> (slots per thread, threads that hold constraints, serial thread, threads)
GEOMETRY = {1: (1, 64, 1, 64), 2: (1, 64, 2, 64), 63: (1, 64, 63, 64), 64: (1, 64, 64, 128), 65: (1, 128, 65, 128),
            448: (1, 448, 448, 512), 449: (1, 512, 449, 512), 511: (1, 512, 511, 512), 512: (2, 256, 256, 320),
            600: (2, 320, 320, 384), 896: (2, 448, 448, 512), 897: (3, 320, 320, 384), 1344: (3, 448, 448, 512),
            1345: (4, 384, 384, 448), 1792: (4, 448, 448, 512), 1793: (5, 384, 384, 448), 2240: (5, 448, 448, 512),
            2241: (6, 384, 384, 448), 2688: (6, 448, 448, 512), 2689: (7, 448, 448, 512), 3136: (7, 448, 448, 512),
            3137: (8, 448, 448, 512), 3584: (8, 448, 448, 512)}
# B: (m, n, R) -- dense_chain_kernel against dense_chain_mw_kernel, bit for bit
B_CASES = ((33, 40, 1040), (600, 40, 48), (2047, 40, 16), (2048, 40, 16), (2689, 40, 16), (3584, 40, 16))
# C: the one-wave kernel beyond eight slots
C_GRID = (3585, 3700, 5055)
C_R = 8
C_EXTRA = (3585, 1040, (0, 17, 1039))
# E: the full driver
E_MS, E_R, E_ZS = (65, 600, 1345), 24, (None, 1, 2, 3, 7)

# csrc/cd_dense.h
DN_GC, DN_SC, DN_FARR_MIN, DN_LDS_WAVE, LDS_BYTES = 64, 32, 4, 2 * 64 + 2 * 32 + 32 + 8, 160 * 1024


def geometry(L, m):
    out4 = (C.c_int * 4)()
    assert L.qcqpmi_dense_chain_geometry(int(m), out4) == 0
    return tuple(out4)


def template_of(SL):
    """The instantiation dense_phase launches for SL slots (csrc/capi_dense.hip)."""
    return 1 if SL <= 1 else 2 if SL <= 2 else 4 if SL <= 4 else 8


def largest_m_one_wave():
    """The largest m whose four per-function arrays (DN_FARR_MIN) plus the lists fit 160 KB of LDS for one wave; m1p = m + 1
    rounded up to a multiple of 64."""
    m1p = (LDS_BYTES // 8 - DN_LDS_WAVE) // DN_FARR_MIN // 64 * 64
    return m1p - 1


# ------------------------------------------------------------------------------------------------ families
def dense_le(n, m):
    """All '<=', all r < 0: scaling a point toward 0 reaches feasibility."""
    from qcqp_amd import problems
    return problems.dense_indefinite(n, m, seed=1000 + m)[0]


def equality_indices(m):
    """Every fifth constraint (k = 1, 6, 11, ...) and the last but one; never the last, the ball."""
    return sorted(set(range(1, m, 5)) | {m - 1})


def dense_mixed(n, m):
    """dense_le with the constraints of equality_indices(m) turned into '==' with r = 0.05 randn."""
    funcs = list(dense_le(n, m))
    rs = np.random.RandomState(2000 + m)
    for k in equality_indices(m):
        P, q, _, _ = funcs[k]
        funcs[k] = (P, q, 0.05 * rs.randn(), '==')
    return funcs


def family(n, m):
    return dense_le(n, m) if m <= 2 else dense_mixed(n, m)


def equalities(funcs):
    return [k for k in range(1, len(funcs)) if funcs[k][3] == '==']


def check_relop_placement(m, eq, geom):
    """'==' in the first and the last-but-one constraint and in every slot j >= 1 of both chain kernels -- except a slot that
    holds the ball alone (the one-wave kernel's last slot when 64 divides m, the multi-wave kernel's when Tc divides m - 1)."""
    eq = set(eq)
    assert 1 in eq and m - 1 in eq and m not in eq
    SL, Tc = geom[0], geom[1]
    if SL <= 8:
        for j in range(1, SL):          # dense_chain_mw_kernel: constraint k is slot (k - 1) // Tc of thread (k - 1) % Tc
            ks = [k for k in range(1 + Tc * j, min(m, Tc * (j + 1)) + 1)]
            assert not ks or ks == [m] or eq & set(ks), (m, 'mw', j)
    top = 0
    for j in range(1, m // 64 + 1):     # dense_chain_kernel: function k is slot k // 64 of lane k % 64
        ks = [k for k in range(64 * j, min(m, 64 * j + 63) + 1)]
        if ks == [m]:
            continue
        assert eq & set(ks), (m, 'one wave', j)
        top = j
    return top      # the highest one-wave slot with an '=='


# ------------------------------------------------------------------------------------------------ starts and traces
def starts(prob, funcs, n, R, restarts=None, seed=3):
    """X1: random points (phase 1).  X2: random directions scaled by 4 (0.7)^j until every '<=' constraint holds (phase 2; the
    slack is then the violation of the '==' constraints).  Only `restarts` are scaled one by one when given; the others take
    the smallest scale found."""
    rs = np.random.RandomState(seed + 7 * len(funcs))
    X1 = 1.5 * rs.randn(n, R)
    X2 = rs.randn(n, R)
    cols = np.arange(R) if restarts is None else np.array(sorted(restarts))
    le = np.array([k for k in range(1, len(funcs)) if funcs[k][3] == '<='])
    a = np.full(len(cols), 4.0)
    for _ in range(100):
        F = prob.eval_batch(X2[:, cols] * a, want_F=True)[2]
        bad = np.max(F[le], axis=0) > 0.0
        if not bad.any():
            break
        a[bad] *= 0.7
    else:
        raise AssertionError('no feasible scale')
    scale = np.full(R, a.min())
    scale[cols] = a
    return X1, X2 * scale


def oracle_traces(orc, prob, X0, phase, restarts, visits):
    """Problem.cd_phase_traced for every compared restart: {r: value of x[i] after each visit}, {r: phase-2 slack}."""
    from conftest import oracle_map

    def one(r):
        rng = orc.Rng(orc.RNG_KEYED, SEED)
        rng.set_restart(FIRST + r)
        _, tr, sl = prob.cd_phase_traced(phase, X0[:, r], visits, rng=rng)
        assert len(tr) == visits, (phase, r, len(tr))
        return tr, 0.0 if sl is None else float(sl)
    res = oracle_map(one, restarts)      # (the trace buffer of the C oracle is per thread)
    return {r: v[0] for r, v in zip(restarts, res)}, {r: v[1] for r, v in zip(restarts, res)}


Case = namedtuple('Case', 'funcs prob n R restarts X trs slack')


def walk_case(orc, m, n=N_FORCED, R=A_R, restarts=None):
    """Problem, starts and the oracle's first sweep of both phases: X[phase], trs[phase][r], slack[phase][r]."""
    funcs = family(n, m)
    prob = orc.Problem(funcs)
    restarts = tuple(range(R)) if restarts is None else tuple(restarts)
    X1, X2 = starts(prob, funcs, n, R, restarts)
    X, trs, slack = {1: X1, 2: X2}, {}, {}
    for phase in (1, 2):
        trs[phase], slack[phase] = oracle_traces(orc, prob, X[phase], phase, restarts, n)
    return Case(funcs, prob, n, R, restarts, X, trs, slack)


def moved_visits(case, blocks):
    """(visits of the walked blocks at which the oracle changes x_i, visits compared)."""
    idx = np.concatenate([np.arange(16 * b, min(16 * b + 16, case.n)) for b in blocks])
    moved = sum(int(np.sum(case.trs[ph][r][idx] != case.X[ph][idx, r])) for ph in (1, 2) for r in case.restarts)
    return moved, 2 * len(idx) * len(case.restarts)


# ------------------------------------------------------------------------------------------------ the walker
Step = namedtuple('Step', 'phase b c r dev start')     # dev: per visited coordinate, relative to 1 + max|start|


def walk(e, case, phase, width, blocks, slack_all=None):
    """Teacher-forced walk along the oracle's first sweep in steps of `width` coordinates (1 or 16) over `blocks`: the engine
    is handed the oracle's states of all compared restarts and runs its unit step (qcqpmi_cd_dense_block_step); the blocks
    left out are taken from the oracle.  Coordinates outside a step must come back untouched.  Returns the steps."""
    n, trs = case.n, case.trs[phase]
    cur = case.X[phase].copy()
    slack = None
    if phase == 2:
        slack = np.zeros(case.R) if slack_all is None else np.array(slack_all, dtype=np.float64)
        for r in case.restarts:
            slack[r] = case.slack[2][r]
    steps = []
    for b in range((n + 15) // 16):
        cnt = min(16, n - 16 * b)
        if b not in blocks:
            for r in case.restarts:
                cur[16 * b:16 * b + cnt, r] = trs[r][16 * b:16 * b + cnt]
            continue
        for c in range(0, cnt, width):
            nc, i0 = min(width, cnt - c), 16 * b + c
            e.upload(cur)
            e.cd_dense_block_step(phase, 0, b, slack=slack, seed=SEED, first_index=FIRST, coords=(c, c + width))
            X1 = e.download()
            rest = np.r_[0:i0, i0 + nc:n]
            for r in case.restarts:
                assert np.array_equal(X1[rest, r], cur[rest, r]), (phase, b, c, r)
                exp = trs[r][i0:i0 + nc]
                dev = np.abs(X1[i0:i0 + nc, r] - exp) / (1.0 + np.max(np.abs(cur[:, r])))
                steps.append(Step(phase, b, c, r, dev, cur[:, r].copy()))
                cur[i0:i0 + nc, r] = exp
    for r in case.restarts:
        assert np.array_equal(cur[:, r], trs[r][:n]), r        # the states that were fed are the oracle's trajectory
    return steps


def self_deviation(orc, case, step, i0, cnt):
    """THE YARDSTICK: the oracle against itself on the visits [i0, i0 + cnt) from start states 1, 32 and 1024 ulps away (every
    coordinate scaled by 1 +- k 2^-52; same draws, same slack): the largest deviation, relative to 1 + max|start|."""
    def visits_from(st):
        rng = orc.Rng(orc.RNG_KEYED, SEED)
        rng.set_restart(FIRST + step.r)
        return case.prob.cd_visits(step.phase, st, 0, i0, cnt, slack2=case.slack[step.phase][step.r], rng=rng)[i0:i0 + cnt]
    base = visits_from(step.start)
    own = 0.0
    for k in (1, 32, 1024):
        for sg in (1.0, -1.0):
            own = max(own, float(np.max(np.abs(visits_from(step.start * (1.0 + sg * k * 2.0 ** -52)) - base))))
    return own / (1.0 + np.max(np.abs(step.start)))


def judge(orc, case, steps, width, strict_first=False):
    """Visit by visit (width 1): every visit within VISIT_TOL of the oracle, or within the yardstick.  Block by block (width 16):
    every block beyond BLOCK_TOL within the yardstick: engine deviation <= 10 x the oracle's own + 1e-6; strict_first: the
    first visit of every block has seen exactly the oracle's state and must be within VISIT_TOL.  Returns (largest deviation,
    largest first-visit deviation, steps that went to the yardstick)."""
    worst, worst_first, judged = 0.0, 0.0, 0
    for s in steps:
        d = float(np.max(s.dev))
        worst, worst_first = max(worst, d), max(worst_first, float(s.dev[0]))
        if strict_first:
            assert s.dev[0] <= VISIT_TOL, (s.phase, s.b, s.c, s.r, s.dev[0])
        if d <= (VISIT_TOL if width == 1 else BLOCK_TOL):
            continue
        judged += 1
        own = self_deviation(orc, case, s, 16 * s.b + s.c, len(s.dev))
        assert d <= 10.0 * own + 1e-6, (s.phase, s.b, s.c, s.r, d, own)
    return worst, worst_first, judged


# ------------------------------------------------------------------------------------------------ D: the lists at capacity
GAP_N, GAP_HALF = 18, 0.25


def gap_centres(name):
    """Centres of the concave constraints -(x_0 - g)^2 + 0.0625 <= 0 (the open gap (g - 0.25, g + 0.25)) and the box of x_0.
    g31 / g32: disjoint gaps, 32 / 33 segments.  g64: 64 gaps that merge into 31 islands (pairs g -+ 0.1, two islands of
    three) -- the gap list exactly full, 32 segments; g65: one gap more than the list holds."""
    if name in ('g31', 'g32'):
        G = int(name[1:])
        return [float(g) for g in range(1, G + 1)], (0.5, G + 0.5)
    cs = [g + d for g in range(1, 32) for d in (-0.1, 0.1)] + [1.0, 2.0]
    if name == 'g65':
        cs.append(3.0)
    assert name in ('g64', 'g65')
    return cs, (0.5, 31.5)


def gap_problem(name, seed=3):
    """n = 18: the box and the gaps on x_0, a ball on all coordinates, one inactive coupling constraint (so the problem is not
    separable), a random indefinite objective."""
    n = GAP_N
    cs, (lo, hi) = gap_centres(name)
    rs = np.random.RandomState(seed)
    A = rs.randn(n, n) / np.sqrt(n)
    funcs = [((A + A.T) / 2.0, rs.randn(n), 0.0, None)]
    E00 = np.zeros((n, n))
    E00[0, 0] = 1.0
    e0 = np.zeros(n)
    e0[0] = 1.0
    funcs.append((E00, -(lo + hi) * e0, lo * hi, '<='))                       # (x_0 - lo) (x_0 - hi) <= 0
    for g in cs:
        funcs.append((-E00, 2.0 * g * e0, -g * g + GAP_HALF ** 2, '<='))       # -(x_0 - g)^2 + 0.0625 <= 0
    rad2 = (hi + 2.0) ** 2 + n
    funcs.append((np.eye(n), np.zeros(n), -rad2, '<='))
    funcs.append((1e-3 * np.ones((n, n)) + np.eye(n), np.zeros(n), -3.0 * rad2, '<='))
    return funcs


def gap_islands(name):
    """The merged gaps, sorted: [(a, b)]."""
    cs, _ = gap_centres(name)
    out = []
    for a, b in sorted((g - GAP_HALF, g + GAP_HALF) for g in cs):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def gap_segments(name):
    """The feasible segments of x_0."""
    _, (lo, hi) = gap_centres(name)
    segs, cur = [], lo
    for a, b in gap_islands(name):
        if a > cur:
            segs.append((cur, min(a, hi)))
        cur = max(cur, b)
    if cur < hi:
        segs.append((cur, hi))
    return segs


def gap_starts(name, R, feasible=True, seed=5):
    """x_0 in the middle of a feasible segment (spread over all of them), or in the middle of an island; the rest small."""
    rs = np.random.RandomState(seed)
    X = 0.3 * rs.randn(GAP_N, R)
    places = gap_segments(name) if feasible else gap_islands(name)
    pick = np.linspace(0, len(places) - 1, R).round().astype(int)
    X[0] = [0.5 * (places[j][0] + places[j][1]) for j in pick]
    return X


def x0_feasible_set(orc, prob, funcs, x, s=0.0):
    """What the chain kernel builds for coordinate 0 at the point x, from orc.feasible_intervals of every constraint:
    (gaps of two-interval constraints that cut into [L, H], segments of [L, H] minus those gaps)."""
    L, H, gaps = -np.inf, np.inf, []
    for k in range(1, len(funcs)):
        t2, t1, t0 = prob.onevar_coeffs(k, x, 0)
        if t2 == 0.0 and t1 == 0.0:
            continue
        iv = orc.feasible_intervals(t2, t1, t0, funcs[k][3], s)
        assert 1 <= len(iv) <= 2
        L, H = max(L, iv[0][0]), min(H, iv[-1][1])
        if len(iv) == 2:
            gaps.append((iv[0][1], iv[1][0]))
    cut = sorted(g for g in gaps if g[1] > L and g[0] <= H)
    nseg, cur = 0, L
    for a, b in cut:
        if a > cur:
            nseg += 1
        cur = max(cur, b)
    if cur < H:
        nseg += 1
    return len(cut), nseg


def in_a_gap(name, x0, margin=1e-9):
    return any(a + margin < x0 < b - margin for a, b in gap_islands(name))
