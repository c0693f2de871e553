"""What tests/test_spectral_wide_cpu.py and tests/test_gpu_spectral_wide.py share (a plain module, no test in it).

jacobi_wide        csrc/jacobi_wide.h in NumPy: the shift c = 2 |A|_F, the round-robin order and hestenes_rotation
                   (csrc/spectral_solve.h), all pairs of a round at once (they own disjoint columns), the stop after the first sweep
                   without a rotation, the normalised columns.  NumPy has no fma and sums a column pairwise: a dot product differs
                   from the kernel's in its last bits, which is what the tolerances of the tests are for.
restate            spectral_wide_kernel stage by stage (csrc/spectral_wide.h): Rayleigh quotients for the eigenvalues, every wave sum
                   as "the lane's two slots first, then wave_sum_tree", then the secular rule and the hard-case rule of
                   spectral_batch_cases (its own secular_root sums 64 lanes, so the root finder is restated here over the two-slot sum).
The families, `case`, `independent`, `scale_of` and `f0` are those of spectral_batch_cases.
"""
import functools

import numpy as np

import spectral_batch_cases as sc

SIZES_WIDE = (65, 66, 95, 96, 127, 128)
MAX_SWEEPS, TOL = sc.MAX_SWEEPS, sc.TOL


def wave_sum2(v):
    """A wave sum over up to 128 values held two per lane (v[l] and v[l + 64]): the two slots first, then the tree of wave_sum_tree."""
    t = np.zeros(128)
    t[:len(v)] = v
    return sc.tree_sum(t[:64] + t[64:])


def hestenes_rotation(alpha, beta, gamma, tol):
    """hestenes_rotation for arrays of pairs: c, s (s == 0.0 exactly: not rotated)."""
    with np.errstate(invalid='ignore'):
        on = np.abs(gamma) > tol * (np.sqrt(alpha) * np.sqrt(beta))
    c, s, _ = sc.rotation(alpha, beta, np.where(on, gamma, 0.0))
    return c, s


@functools.lru_cache(maxsize=None)
def rounds_of(n2):
    return [np.array([sc.round_robin_pair(n2, r, k) for k in range(n2 // 2)]) for r in range(n2 - 1)]


def jacobi_wide(A, max_sweeps=MAX_SWEEPS, tol=TOL):
    """jacobi_wide on a copy of A (n x n, any n >= 1): (U with COLUMN k = u_k including the padding coordinate (n2 x n2), sweeps,
    converged, c)."""
    n = A.shape[0]
    n2 = (n + 1) & ~1
    G = np.zeros((n2, n2))
    G[:n, :n] = A
    fro2 = wave_sum2(np.sum(G * G, axis=0))
    if fro2 == 0.0:
        return np.eye(n2), 0, True, 0.0
    c = 2.0 * np.sqrt(fro2)
    G[np.arange(n2), np.arange(n2)] += c
    sweeps, converged = 0, False
    while sweeps < max_sweeps:
        rotated = False
        for pq in rounds_of(n2):
            p, q = pq[:, 0], pq[:, 1]
            gp, gq = G[:, p], G[:, q]
            cr, sr = hestenes_rotation(np.einsum('ij,ij->j', gp, gp), np.einsum('ij,ij->j', gq, gq), np.einsum('ij,ij->j', gp, gq), tol)
            if np.any(sr != 0.0):
                rotated = True
                G[:, p], G[:, q] = cr * gp - sr * gq, sr * gp + cr * gq
        sweeps += 1
        if not rotated:
            converged = True
            break
    return G / np.sqrt(np.einsum('ij,ij->j', G, G)), sweeps, converged, c


def degenerate_norm(A):
    """JacobiWideResult::degenerate of csrc/jacobi_wide.h: A has a nonzero entry but fro2, summed as the solver sums it, comes out as
    0.0 (the solver's zero-matrix exit, taken wrongly) or is not finite (c = inf).  Status 2."""
    with np.errstate(over='ignore', under='ignore'):
        fro2 = wave_sum2(np.sum(A * A, axis=0))
    return bool(not fro2 < np.inf or (fro2 == 0.0 and np.any(A != 0.0)))


def secular_root(gh, d, rho, lo, hi):
    """secular_root of csrc/spectral_solve.h with the sums of the wide kernel."""
    rho2 = rho * rho
    hi = max(hi, lo)
    sigma, it = lo, 0
    while True:
        den = d + sigma
        w = sc._w(gh, den)
        psi = wave_sum2(w * w)
        with np.errstate(divide='ignore', invalid='ignore'):
            T = wave_sum2(np.where(w == 0.0, 0.0, w * w / den))
        it += 1
        sq = np.sqrt(psi)
        if abs(sq - rho) <= sc.SECULAR_RTOL * rho or it >= sc.SECULAR_MAX_ITERS:
            break
        if psi > rho2:
            lo = sigma
        else:
            hi = sigma
        with np.errstate(divide='ignore', invalid='ignore'):
            nxt = sigma + (psi / T) * ((sq - rho) / rho)
        if not (nxt > lo and nxt < hi):
            nxt = 0.5 * (lo + hi)
        if nxt == sigma:
            break
        sigma = nxt
    return sigma, it


def restate(P0, q0, r0, agg, relop, max_sweeps=MAX_SWEEPS, tol=TOL):
    """One problem as spectral_wide_kernel solves it; the dictionary of spectral_batch_cases.restate (and U, the eigenvectors)."""
    n = q0.size
    eq = relop == '=='
    a, beta, gamma = agg[:n], agg[n:2 * n], agg[2 * n]
    s = np.sqrt(a)
    h = beta / (2.0 * a)
    A = P0 / (s[:, None] * s[None, :])
    ph = P0.T.dot(h)
    rho2 = wave_sum2(beta * beta / (4.0 * a)) - gamma
    rho = np.sqrt(rho2)
    g = (0.5 * q0 - ph) / s
    U2, sweeps, conv, _ = jacobi_wide(A, max_sweeps, tol)
    U = U2[:n, :n]
    lam = np.einsum('ik,ik->k', U, A.dot(U))
    gh = U.T.dot(g)
    order = np.lexsort((np.arange(n), lam))
    kmin = int(order[0])
    lam_min, lam_abs = float(lam[kmin]), float(np.max(np.abs(lam)))
    d = lam - lam_min
    g2 = wave_sum2(gh * gh)
    branch, sigma, tau, mu = 1, 0.0, 0.0, 0.0
    interior = False
    if not eq and lam_min > 0.0:
        w = sc._w(gh, lam)
        interior = wave_sum2(w * w) <= rho2
    if interior:
        branch, w = 0, -w
    else:
        sigma_lo = lam_min if (not eq and lam_min > 0.0) else 0.0
        hard = 0
        if sigma_lo == 0.0:
            inL = d <= sc.HARD_THR * lam_abs
            w0 = sc._w(gh, d)
            wr = np.where(inL, 0.0, w0)
            gL2 = wave_sum2(np.where(inL, gh * gh, 0.0))
            psi_reg, psi0 = wave_sum2(wr * wr), wave_sum2(w0 * w0)
            if gL2 <= sc.HARD_THR * sc.HARD_THR * g2 and psi_reg <= rho2:
                hard = 1
            elif psi0 <= rho2:
                hard = 2
        if hard:
            branch = 2
            w = -(wr if hard == 1 else w0)
            tau = np.sqrt(rho2 - (psi_reg if hard == 1 else psi0))
        else:
            lo = max(sigma_lo, float(np.max(np.abs(gh) / rho - d)))
            sigma, _ = secular_root(gh, d, rho, lo, np.sqrt(g2) / rho)
            w = -sc._w(gh, d + sigma)
        mu = sigma - lam_min
    y = U.dot(w)
    if branch == 2:
        v = U[:, kmin]
        lead = v[int(np.argmax(np.abs(v)))]
        y = y + (-tau if lead < 0.0 else tau) * v
    x = (y - beta / (2.0 * s)) / s
    bound = wave_sum2(x * (P0.T.dot(x) + q0)) + r0
    status = 2 if degenerate_norm(A) else (0 if conv else 1)
    return dict(x=x, bound=bound, mu=mu, lam=lam[order], sweeps=sweeps, branch=branch, status=status, y=y, rho=rho, A=A, g=g, U=U2)


@functools.lru_cache(maxsize=None)
def restated(name, n, B, seed=3):
    fl, P0s, q0s, r0s, aggs, relop, _ = sc.case(name, n, B, seed)
    return [restate(P0s[b], q0s[b], r0s[b], aggs[b], relop) for b in range(B)]
