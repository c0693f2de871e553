"""What tests/test_admm_batch_cpu.py and tests/test_gpu_admm_batch.py share: the grid of qcqpmi_admm_small_batch_run's domain (families,
sizes, batch sizes, seeds), the oracle's improve_admm with its iteration counts, the perturbation of the sensitivity check and the
arguments that aim at every exit of the iteration.  A plain module, not a conftest: the test files import what they use.

The horizon.  On constraints x_i^2 == d the ADMM iteration doubles a last-bit difference with every iteration (1e-9
after 10 + 10 iterations at n = 17, 1e-6 after 20 + 20 at n = 63, measured with the oracle alone), so restart-by-restart parity is
asserted at NUM_ITERS = 5 per phase, where the oracle itself moves by at most 5e-12 under a last-bit perturbation of the starts of
this grid (tests/test_admm_batch_cpu.py asserts 1e-11)."""
import itertools

import numpy as np

from sdr_batch_cases import objectives      # noqa: F401  (P0s, q0s, r0s of a list of problems)
from small_batch_pc_cases import FAMILIES as PC_FAMILIES, MAXC4 as PC_MAXC4, cons_of, family as pc_family      # noqa: F401

NS = (1, 2, 7, 16, 17, 31, 32, 33, 48, 63, 64)
BRS = list(itertools.product((1, 3, 17), (1, 5, 17)))
FAMILIES = ('bls', 'cut', 'box', 'lin2', 'ann2')
MAXC4 = ('lin2', 'ann2')                    # two constraints on a coordinate: the <4> kernels
PC_NS = (7, 33, 64)
NUM_ITERS = 5                               # per phase: the stable horizon
EPS = 4e-16                                 # relative size of the perturbation of a start
SENSITIVITY = 1e-11                         # what the oracle may move by under it: a hundredth of the GPU threshold
PARITY = 1e-9
# (family, n) -> problem seed that replaces the rule's (3 + index of n); none was needed
RESEEDED = {}


def family(name, n, B, seed=1):
    """B problems of the family: shared separable constraints, B objectives (problem b from seed + b)."""
    from qcqp_amd import problems
    if name == 'bls':
        return problems.boolean_least_squares_batch(B, n, n + n // 2 + 1, seed=seed)
    if name == 'cut':          # weighted MAXCUT: an indefinite objective with zero diagonal, q0 = 0
        cons = problems.maxcut(n, seed=seed, weighted=True)[0][1:]
        return [[problems.maxcut(n, seed=seed + b, weighted=True)[0][0]] + cons for b in range(B)]
    if name == 'box':          # (x_i + 1)(x_i - 1) <= 0 under an objective with an indefinite diagonal
        return problems.box_qp_batch(n, [seed + b for b in range(B)])
    if name in ('lin2', 'ann2'):      # two linear constraints per coordinate; annulus pair on even, equality on odd coordinates
        cons = problems.multi_class(name, n, seed=seed)[1:]
        return [[problems.multi_class(name, n, seed=seed + b)[0]] + cons for b in range(B)]
    raise KeyError(name)


def cases():
    """(family, n, B, R, problem seed, seed, seed_stride, first_index): every n with every family, the nine (B, R) pairs dealt
    round-robin."""
    out = []
    for k0, name in enumerate(FAMILIES):
        for j, n in enumerate(NS):
            B, R = BRS[(k0 + 2 * j) % len(BRS)]
            out.append((name, n, B, R, RESEEDED.get((name, n), 3 + j), 11 + j + 100 * k0, 3, 5 * j))
    return out


def pc_cases():
    """(family, n, B, R, problem seed, seed, seed_stride, first_index) of the per-problem-coefficient families."""
    out = []
    for k0, name in enumerate(PC_FAMILIES):
        for j, n in enumerate(PC_NS):
            out.append((name, n, 3, 5, 40 + 10 * j + k0, 23 + j + 100 * k0, 3, 5 * j))
    return out


def case_id(c):
    return '%s-n%d-B%d-R%d' % c[:4]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if a.size else 0.0


def seed_of(seed, stride, b):
    return (seed + b * stride) % 2 ** 64


def starts(orc, seed, stride, first_index, B, R, n):
    """X0 (B, R, n): the keyed normals (seed + b stride, first_index + r, j) the kernel draws."""
    return np.stack([orc.keyed_normal_matrix(seed_of(seed, stride, b), n, R, first_index).T for b in range(B)])


def perturbed(X0):
    """Every entry moved by a relative EPS, signs alternating."""
    sg = np.where(np.arange(X0.size).reshape(X0.shape) % 2 == 0, 1.0, -1.0)
    return X0 * (1.0 + EPS * sg)


def improve_admm(prob, x0, num_iters=1000, viol_lim=1e4, tol=1e-2, rho=None, phase1=True):
    """oracle.Problem.improve_admm (qcqp.py:254-285) with the iteration counts of its two phases: (x, iters1, iters2)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    if rho is None:
        rho = prob.auto_rho()
    it1 = 0
    if phase1:
        z1, it1 = prob.admm_phase1(x0, tol, num_iters)
        x1 = x0 if prob.better(x0, z1) == 1 else z1
    else:
        x1 = x0
    z2, it2 = prob.admm_phase2(x1, rho, tol, num_iters, viol_lim)
    return (x1 if prob.better(x1, z2) == 1 else z2), it1, it2


def oracle_batch(orc, oracle_map, fl, X0, rhos=None, **kw):
    """improve_admm of every (problem, restart): X (B, R, n), iters1, iters2, f0, maxviol (B, R)."""
    B, R, n = X0.shape
    probs = [orc.Problem(f) for f in fl]
    for p in probs:
        p.eig()                  # once per problem, before the threads share it

    def one(br):
        b, r = divmod(br, R)
        x, i1, i2 = improve_admm(probs[b], X0[b, r], rho=None if rhos is None else float(rhos[b]), **kw)
        return x, i1, i2, probs[b].eval(0, x), probs[b].max_violation(x)
    res = oracle_map(one, range(B * R))
    X = np.array([q[0] for q in res]).reshape(B, R, n)
    cols = [np.array([q[k] for q in res]).reshape(B, R) for k in (1, 2, 3, 4)]
    return X, cols[0], cols[1], cols[2], cols[3]


# ---- the cases that aim at an exit of the iteration; every one runs NUM_ITERS iterations per phase at the most

def feasible_starts(name, n, R, seed):
    """Starts on which phase 1 stops at t = 0: +-1 points for bls, interior points for box."""
    rs = np.random.RandomState(seed)
    if name == 'bls':
        return np.where(rs.uniform(size=(R, n)) < 0.5, -1.0, 1.0)
    return rs.uniform(-0.9, 0.9, size=(R, n))


def exit_cases():
    """(label, family, n, problem seed, keyword arguments, what the iteration counts must be: a function of (iters1, iters2))."""
    N = NUM_ITERS
    return [
        ('phase1-at-0-bls', 'bls', 17, 5, dict(num_iters=N), lambda i1, i2: np.all(i1 == 0)),
        ('phase1-at-0-box', 'box', 33, 6, dict(num_iters=N), lambda i1, i2: np.all(i1 == 0)),
        ('no-phase1', 'bls', 32, 7, dict(num_iters=N, phase1=False), lambda i1, i2: np.all(i1 == 0) and np.all(i2 >= 1)),
        ('phase2-by-tol', 'cut', 31, 8, dict(num_iters=N, tol=1e3), lambda i1, i2: np.all(i2 == 2)),
        ('phase2-by-viol-lim', 'bls', 48, 9, dict(num_iters=N, viol_lim=1e-9), lambda i1, i2: np.all(i2 == 1)),
        ('one-iteration', 'ann2', 16, 10, dict(num_iters=1), lambda i1, i2: np.all(i1 <= 1) and np.all(i2 == 1)),
    ]


EXIT_R = 6
WINNER_CASES = ((33, 2), (33, 4))           # (n, seed) of box_qp on which the start below wins both comparisons
WINNER_KW = dict(num_iters=NUM_ITERS, tol=1e-6)


def winning_start(orc, n, seed):
    """A start that wins both `better` comparisons of improve_admm on box_qp(n, seed): a good point of the box (300 + 300 iterations
    of the oracle from a normal start) whose coordinates at a bound are pushed 2e-5 outside -- violation 4e-5, in the bucket of the
    feasible points, and a lower objective than any of them nearby.  With tol = 1e-6 phase 1 runs and phase 2 runs, and neither
    finds a point `better` prefers.  Returns (funcs, x0)."""
    from qcqp_amd import problems
    funcs = problems.box_qp(n, seed=seed)[0]
    prob = orc.Problem(funcs)
    xs, _, _ = improve_admm(prob, np.random.RandomState(seed).randn(n), num_iters=300)
    act = np.abs(np.abs(xs) - 1.0) < 1e-3
    x0 = xs.copy()
    x0[act] = np.sign(xs[act]) * (1.0 + 2e-5)
    return funcs, x0
