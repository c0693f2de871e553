// Scalar pieces of the batched spectral suggest (spectral_small.hip) and of the symmetric Jacobi eigen-solver it runs on
// (jacobi_small.h), in a header that is also plain C++ (no HIP include; build the host side with -ffp-contract=off like the device
// side), so that a host program can drive them: tests/host/spectral_selftest.cpp.
//
//   jacobi_rotation     the rotation that annihilates a_pq of a symmetric 2 x 2 block
//   hestenes_rotation   the rotation that makes two columns orthogonal (one-sided Jacobi, jacobi_wide.h), behind its threshold
//   round_robin_pair    the pair of (round, slot) in the cyclic ordering: n2 / 2 disjoint pairs per round, every pair once per sweep
//   tree_sum64          the order of wave_sum_tree (dev_util.h) over an array of 64
//   secular_root        the root of  psi(sigma) = sum_k gh_k^2 / (d_k + sigma)^2 = rho^2  by a safeguarded Newton iteration
//   spectral_hard_case  the rule that separates the hard case of the trust-region problem from the regular one
//
// THE SECULAR EQUATION.  With lam ascending in value (any index order), d_k = lam_k - lam_min >= 0 and sigma = mu + lam_min the
// boundary solution of  min y'Ay + 2 g'y  s.t. |y| = rho  is y = -Q (gh / (d + sigma)) at the sigma >= 0 with psi(sigma) = rho^2.
// phi(sigma) = 1 / sqrt(psi) - 1 / rho is concave and increasing on sigma > 0, so Newton's iteration on phi from a point LEFT of the
// root rises to it monotonically and never passes it; the start
//        sigma_0 = max(sigma_lo, max_k (|gh_k| / rho - d_k))                  (every single term of psi is at most rho^2 at the root)
// is such a point, and sqrt(sum gh^2) / rho is right of it.  The rule, fixed: evaluate psi and T = sum gh^2 / (d + sigma)^3; move the
// bracket end on sigma's side; stop when |sqrt(psi) - rho| <= SECULAR_RTOL rho; take sigma + (psi / T) (sqrt(psi) - rho) / rho, or
// the bracket's midpoint where that step leaves the open bracket (or is a NaN); stop when the step does not move sigma or after
// SECULAR_MAX_ITERS evaluations.  A term with gh_k == 0 is 0 whatever its denominator.
//
// THE HARD CASE.  L = {k : d_k <= SPECTRAL_HARD_THR max|lam|} is the lowest eigenspace as far as double precision tells.  With
//        gL2 = sum_{k in L} gh_k^2,   g2 = sum_k gh_k^2,   psi_reg = sum_{k not in L} (gh_k / d_k)^2,   psi_0 = sum_k (gh_k / d_k)^2
// (a term with gh_k == 0 is 0; gh_k != 0 over d_k == 0 is +inf) the problem is treated as the hard case -- mu = -lam_min,
// y = y_reg + tau q_min, tau = sqrt(rho^2 - |y_reg|^2) -- when
//        (gL2 <= SPECTRAL_HARD_THR^2 g2  and  psi_reg <= rho^2)       the components in L are dropped: y_reg over k not in L    (1)
//   or   psi_0 <= rho^2                                               nothing is dropped: psi has no root right of 0          (2)
// SPECTRAL_HARD_THR = 2^-46 (1.4e-14): the rounding of gh = Q'g is about n eps |g| (7e-15 |g| at n = 64), so a component below the
// threshold carries no sign that could be trusted.  Dropping it leaves a stationarity residual of at most 2^-46 |g|, five orders
// below the 1e-9 of the certificates; on the regular side sigma >= |gh_L| / rho > 2^-46 |g| / rho is far from underflow.  The VALUE
// is continuous across the threshold: the two treatments differ by 2 |gh_L| tau <= 2^-45 |g| rho in the objective.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SPS_FN __host__ __device__ inline
#else
#define SPS_FN inline
#endif

namespace qcqpmi {

constexpr double SPECTRAL_HARD_THR = 0x1p-46;
constexpr double SECULAR_RTOL = 0x1p-50;       // 4 eps: |y| = rho to four units in the last place
constexpr int SECULAR_MAX_ITERS = 200;

// J = [[c, s], [-s, c]] on (p, q), p < q:  J' [[app, apq], [apq, aqq]] J is diagonal with a_pp' = app - t apq, a_qq' = aqq + t apq.
// theta = (aqq - app) / (2 apq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (the smaller root: |t| <= 1; theta == 0: t = 1),
// c = 1 / sqrt(t^2 + 1), s = t c.  apq == 0: the identity.  A theta whose square overflows gives t = 0 through 1 / inf.
struct JacobiRot { double c, s, t; };

SPS_FN JacobiRot jacobi_rotation(double app, double aqq, double apq) {
    JacobiRot r = {1.0, 0.0, 0.0};
    if (apq == 0.0) return r;
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = fabs(theta);
    double t = 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    r.c = 1.0 / sqrt(t * t + 1.0);
    r.s = t * r.c;
    r.t = t;
    return r;
}

// The rotation of ONE-SIDED (Hestenes) Jacobi on two columns g_p, g_q (p < q) of G, from alpha = g_p . g_p, beta = g_q . g_q and
// gamma = g_p . g_q:  (g_p, g_q) <- (c g_p - s g_q, s g_p + c g_q) makes the columns orthogonal and keeps alpha + beta.  It is
// jacobi_rotation of the 2 x 2 Gram block [[alpha, gamma], [gamma, beta]] (theta = (beta - alpha) / (2 gamma); theta == 0: t = 1)
// behind a relative threshold: the pair is rotated only where |gamma| > tol sqrt(alpha) sqrt(beta) (the two roots apart: the product
// alpha beta may overflow or underflow where its root does not).  Otherwise -- gamma == 0, or a NaN among the three -- the identity
// with s == 0 exactly, which the caller reads as "not rotated".
SPS_FN JacobiRot hestenes_rotation(double alpha, double beta, double gamma, double tol) {
    const JacobiRot id = {1.0, 0.0, 0.0};
    if (!(fabs(gamma) > tol * (sqrt(alpha) * sqrt(beta)))) return id;
    return jacobi_rotation(alpha, beta, gamma);
}

// The circle method over n2 players (n2 even, >= 2), m = n2 - 1: in round r (0 <= r < m) slot 0 pairs player m with player r and
// slot k (1 <= k < n2 / 2) pairs (r + k) mod m with (r - k) mod m.  The n2 / 2 pairs of a round are disjoint and the m rounds hold
// every pair exactly once.  Returned with p < q.
SPS_FN void round_robin_pair(int n2, int round, int slot, int *p, int *q) {
    const int m = n2 - 1;
    int a, b;
    if (slot == 0) {
        a = m; b = round;
    } else {
        a = (round + slot) % m;
        b = (round - slot + m) % m;
    }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// v[0..63] summed as wave_sum_tree sums the lanes: the binary tree over adjacent entries (pairs, quads, eights, ...)
SPS_FN double tree_sum64(const double *v) {
    double t[64];
    for (int i = 0; i < 64; i++) t[i] = v[i];
    for (int w = 64; w > 1; w >>= 1)
        for (int i = 0; i < w / 2; i++) t[i] = t[2 * i] + t[2 * i + 1];
    return t[0];
}

// one component of y (up to sign) and its share of psi and T
SPS_FN double secular_w(double gh, double den) { return gh == 0.0 ? 0.0 : gh / den; }

// psi and T over arrays of n <= 64 (the host's evaluation; the kernel forms the same terms per lane and sums with wave_sum_tree)
SPS_FN void secular_eval(int n, const double *gh, const double *d, double sigma, double *psi, double *T) {
    double a[64], b[64];
    for (int k = 0; k < 64; k++) {
        const double den = k < n ? d[k] + sigma : 1.0;
        const double w = k < n ? secular_w(gh[k], den) : 0.0;
        a[k] = w * w;
        b[k] = w == 0.0 ? 0.0 : w * w / den;
    }
    *psi = tree_sum64(a);
    *T = tree_sum64(b);
}

struct SecularRoot { double sigma, psi; int iters; };

// eval(sigma, &psi, &T).  lo: sigma_0 above (left of the root or on it); hi: a point right of the root (taken as at least lo).
template <class Eval>
SPS_FN SecularRoot secular_root(Eval eval, double rho, double lo, double hi) {
    SecularRoot r;
    const double rho2 = rho * rho;
    if (!(hi > lo)) hi = lo;
    double sigma = lo, psi = 0.0, T = 0.0;
    int it = 0;
    for (;;) {
        eval(sigma, &psi, &T);
        it++;
        const double sq = sqrt(psi);
        if (fabs(sq - rho) <= SECULAR_RTOL * rho || it >= SECULAR_MAX_ITERS) break;
        if (psi > rho2) lo = sigma; else hi = sigma;
        double next = sigma + (psi / T) * ((sq - rho) / rho);
        if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
        if (next == sigma) break;
        sigma = next;
    }
    r.sigma = sigma; r.psi = psi; r.iters = it;
    return r;
}

// the whole root finder over arrays (the host's)
SPS_FN SecularRoot secular_solve(int n, const double *gh, const double *d, double rho, double sigma_lo) {
    double g2[64], lo = sigma_lo;
    for (int k = 0; k < 64; k++) g2[k] = k < n ? gh[k] * gh[k] : 0.0;
    for (int k = 0; k < n; k++) {
        const double c = fabs(gh[k]) / rho - d[k];
        if (c > lo) lo = c;
    }
    const double hi = sqrt(tree_sum64(g2)) / rho;
    return secular_root([=](double s, double *psi, double *T) { secular_eval(n, gh, d, s, psi, T); }, rho, lo, hi);
}

// 0: regular; 1: hard, the components in L dropped (rule 1); 2: hard, nothing dropped (rule 2)
SPS_FN int spectral_hard_case(double gL2, double g2, double psi_reg, double psi0, double rho2) {
    if (gL2 <= SPECTRAL_HARD_THR * SPECTRAL_HARD_THR * g2 && psi_reg <= rho2) return 1;
    if (psi0 <= rho2) return 2;
    return 0;
}

}  // namespace qcqpmi
