"""What tests/test_admm_wide_cpu.py and tests/test_gpu_admm_wide.py share: the grid of qcqpmi_admm_batch_run's wide domain (65 <= n <=
128: families, sizes, batch sizes, seeds), built from the pieces of admm_batch_cases -- the same families, the same keyed starts, the
same perturbation, the same horizon NUM_ITERS = 5 per phase and the same two thresholds (the oracle moves by <= SENSITIVITY = 1e-11,
the GPU agrees to PARITY = 1e-9).  A plain module, not a conftest: the test files import what they use.

The sizes: 65 and 66 put one and two live lanes into slot 1 (lane l holds coordinates l and l + 64); 95, 96, 97 lie around the 64 KB
LDS image (from n = 91 the launch raises the dynamic LDS limit); 127 and 128 fill slot 1."""
import itertools

import numpy as np

from admm_batch_cases import (FAMILIES, MAXC4, NUM_ITERS, PARITY, PC_FAMILIES, PC_MAXC4, SENSITIVITY, case_id, cons_of, family,      # noqa: F401
                              feasible_starts, improve_admm, objectives, oracle_batch, pc_family, perturbed, rel, seed_of, starts,
                              winning_start, EXIT_R, WINNER_KW)
from small_batch_pc_cases import entry

NS = (65, 66, 95, 96, 97, 127, 128)
BRS = list(itertools.product((1, 3), (1, 5, 9)))      # R = 9: more restarts than the eight waves of a workgroup
PC_NS = (65, 96, 128)
# (family, n) -> problem seed that replaces the rule's (3 + index of n); none was needed
RESEEDED = {}


def cases():
    """(family, n, B, R, problem seed, seed, seed_stride, first_index): every n with every family, the six (B, R) pairs dealt
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


def exit_cases():
    """(label, family, n, problem seed, keyword arguments, what the iteration counts must be: a function of (iters1, iters2))."""
    N = NUM_ITERS
    return [
        ('phase1-at-0-bls', 'bls', 81, 5, dict(num_iters=N), lambda i1, i2: np.all(i1 == 0)),
        ('phase1-at-0-box', 'box', 97, 6, dict(num_iters=N), lambda i1, i2: np.all(i1 == 0)),
        ('no-phase1', 'bls', 96, 7, dict(num_iters=N, phase1=False), lambda i1, i2: np.all(i1 == 0) and np.all(i2 >= 1)),
        ('phase2-by-tol', 'cut', 95, 8, dict(num_iters=N, tol=1e3), lambda i1, i2: np.all(i2 == 2)),
        ('phase2-by-viol-lim', 'bls', 112, 9, dict(num_iters=N, viol_lim=1e-9), lambda i1, i2: np.all(i2 == 1)),
        ('one-iteration', 'ann2', 80, 10, dict(num_iters=1), lambda i1, i2: np.all(i1 <= 1) and np.all(i2 == 1)),
    ]


def exit_starts(orc, e):
    """The starts X0 (2, EXIT_R, n) of an exit case and the arguments that make the kernel take them (X0, or the keyed seed)."""
    label, name, n, ps = e[:4]
    if label.startswith('phase1-at-0'):
        X0 = np.stack([feasible_starts(name, n, EXIT_R, ps + b) for b in range(2)])
        return X0, dict(X0=X0)
    return starts(orc, 31, 3, 0, 2, EXIT_R, n), dict(seed=31, stride=3)


WINNER_CASES = ((97, 2), (128, 2))           # (n, seed) of box_qp on which winning_start wins both comparisons

FREE_N = 100
FREE_CASES = ((80,), (10, 80))               # coordinates left without a constraint: one in slot 1 only, one in each slot


def free_family(free, B, seed=13):
    """B Boolean least squares problems of FREE_N variables whose constraints on the coordinates `free` are dropped (m = n - len(free))."""
    fl = family('bls', FREE_N, B, seed=seed)
    keep = [k for k, (P, q, _, _) in enumerate(fl[0][1:]) if entry(P, q)[0] not in free]
    assert len(keep) == FREE_N - len(free)
    return [[f[0]] + [f[1 + k] for k in keep] for f in fl]


FREE_R, FREE_SEED = 5, 41
