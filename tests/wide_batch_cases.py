"""What tests/test_wide_batch_cpu.py and tests/test_gpu_wide_batch.py share: the sizes of the wide batch (65 <= n <= 128, two
coordinates per lane), the batch shapes and the seeds of every grid case.  A plain module, not a conftest: the test files import
what they use."""
import itertools

NW = (65, 66, 95, 96, 97, 127, 128)      # one coordinate in slot 1; around the half; lane 63 without a second coordinate; full
NW_PC = (65, 96, 128)
BR = list(itertools.product((1, 3, 33), (1, 5, 17)))
SHARED = ('bls', 'box01', 'box11', 'box01neg', 'box11neg', 'eq2', 'ann2', 'cut')
ITERS = 1000

# (family, n) -> (family seed, restart seed) of the CPU pin; a case that the pin shows to be chaotic gets another pair HERE (the
# tolerance and the coverage stay).  None needed one.
CPU_SEEDS = {}


def cpu_seeds(name, n):
    return CPU_SEEDS.get((name, n), (5, 77))


def grid_case(k0, j, n):
    """Case j (size n) of family number k0: (B, R, family seed, seed, seed stride, first index) -- the nine (B, R) pairs dealt
    round-robin, so that every family meets every B and every R."""
    B, R = BR[(k0 + j) % len(BR)]
    return B, R, 3 + j, 11 + j, 3, 5 * j
