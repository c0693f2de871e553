"""What tests/test_sdr_wide_cpu.py and tests/test_gpu_sdr_wide.py share: the grid of the wide range of qcqpmi_sdr_batch (65 <= n <=
128: families, sizes, batch sizes, seeds) and a NumPy restatement of sdr_small_kernel<true> that performs its sweeps in the kernel's
exact order (csrc/sdr_small.h): C_b read from the packed lower triangle, the row product as four partial sums over j mod 4, the wave
sums as the binary tree.  The families, the lifted cost, the keyed start, the stacked restatement mixing_numpy and the certificate
come from tests/sdr_batch_cases.py.  A plain module, not a conftest: the test files import what they use."""
import itertools

import numpy as np

import sdr_batch_cases as sc

NS = (65, 66, 95, 96, 97, 127, 128)             # N = n + 1: N mod 4 = 2, 3, 0, 1, 2, 0, 1; both ends and the middle of the wide range
BS = list(itertools.product((1, 3), (1, 17, 64)))
FAMILIES = sc.FAMILIES
TOL, MAX_SWEEPS = 1e-13, 20000
K = sc.K
# problem seeds that replace the rule's (3 + index of n): scaled, n = 127 at seed 8 holds a problem (the third of the batch) that the
# NumPy restatement leaves at the sweep limit (lambda_min / scale -2.7e-09 there); 40: 2336 sweeps at most, lambda_min / scale >= -1.4e-08
RESEEDED = {('scaled', 127): 40}


def cases():
    """(family, n, B, S, problem seed, seed, seed_stride, first_index): every n with every family; the six (B, S) pairs dealt
    round-robin along n, shifted by two from family to family -- every family meets all six pairs, so every B and every S."""
    out = []
    for k0, name in enumerate(FAMILIES):
        for j, n in enumerate(NS):
            B, S = BS[(2 * k0 + j) % len(BS)]
            out.append((name, n, B, S, RESEEDED.get((name, n), 3 + j), 11 + j + 100 * k0, 3, 5 * j))
    return out


def tri(i):
    return i * (i + 1) // 2


def pack(C):
    """The lower triangle with the diagonal, row after row: C_ij at tri(max(i, j)) + min(i, j)."""
    N = C.shape[0]
    return np.concatenate([C[i, :i + 1] for i in range(N)])


def packed_row_product(Cp, V, N, i):
    """g (64,) = sum_{j != i} C_ij V[j]: four partial sums over j = 0, 1, 2, 3 (mod 4) in ascending j over the full fours, what is left
    of N after the last full four to the first; the term j == i adds 0.0 V[j]; (a0 + a1) + (a2 + a3).  (The kernel's fma rounds once
    where the product and the sum here round twice: last bits.)"""
    a = np.zeros((4, V.shape[1]))
    full = N - N % 4
    for j in range(N):
        c = 0.0 if j == i else Cp[tri(i) + j if j < i else tri(j) + i]
        r = j % 4 if j < full else 0
        a[r] = c * V[j] + a[r]
    return (a[0] + a[1]) + (a[2] + a[3])


def exact_sweeps(C, V0, k):
    """k sweeps of ONE problem (C (N, N) symmetric, V0 (N, 64)) with tol = 0 in the order of the kernel.  Returns (V, the tracked
    objective -- the first pass's value plus the exact decrease of every update --, the objective recomputed at the end, y)."""
    N = C.shape[0]
    Cp = pack(C)
    assert Cp.size == N * (N + 1) // 2
    V = np.array(V0, dtype=np.float64)

    def objective():
        f, y = 0.0, np.empty(N)
        for i in range(N):
            g = packed_row_product(Cp, V, N, i)
            t = sc.tree_sum(g * V[i]) + Cp[tri(i) + i] * sc.tree_sum(V[i] * V[i])
            f += t
            y[i] = -t
        return f, y

    f = objective()[0]
    for _ in range(k):
        dsweep = 0.0
        for i in range(N):
            g = packed_row_product(Cp, V, N, i)
            gv = sc.tree_sum(g * V[i])
            nrm = np.sqrt(sc.tree_sum(g * g))
            if nrm > 0.0:
                V[i] = -g / nrm
                dsweep += -2.0 * (nrm + gv)
        f += dsweep
    primal, y = objective()
    return V, f, primal, y
