// The host-compilable pieces of the batched spectral suggest (qcqp_amd/csrc/spectral_solve.h) against long-double references, on
// random and degenerate inputs.  Built by tests/test_spectral_batch_cpu.py with the host compiler, -ffp-contract=off (the device
// build's setting) and tests/host/hip_stub; prints "ok <checks>" or the first failure.
//   rotation     c^2 + s^2 = 1, the rotated off-diagonal entry vanishes and a_pp' = app - t apq is the rotated diagonal entry, all in
//                long double; a_pq = 0 is the identity; equal diagonal entries give t = +-1; a huge theta gives t = 0 without a NaN
//   round robin  for every even n2 <= 64: the pairs of a round are disjoint and a sweep visits every pair exactly once
//   tree sum     the order of the binary tree over adjacent entries, written out
//   Jacobi       the sweep of jacobi_small.h restated on the host from the two pieces: A Q' = Q' diag(lam) in long double, the trace
//                and the Frobenius norm kept; random matrices, the identity, a repeated lowest eigenvalue, equal diagonal entries
//   secular      psi(sigma) = rho^2 in long double at the root of secular_solve; gh with zeros, gh = 0 on a repeated lowest
//                eigenvalue, a root many orders below the spectrum's scale; the hard-case rule on both sides of its threshold
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spectral_solve.h"

using namespace qcqpmi;

static long checks = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        checks++;                                                                         \
        if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double urand() {      // xorshift64*, (0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return ((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-17;
}
static double nrand() { return sqrt(-2.0 * log(urand())) * cos(6.283185307179586 * urand()); }

static void check_rotation(double app, double aqq, double apq) {
    const JacobiRot r = jacobi_rotation(app, aqq, apq);
    const long double c = r.c, s = r.s, t = r.t;
    const long double sc = fabsl((long double)app) + fabsl((long double)aqq) + fabsl((long double)apq);
    CHECK(std::isfinite(r.c) && std::isfinite(r.s) && std::isfinite(r.t), "app %g aqq %g apq %g", app, aqq, apq);
    CHECK(fabsl(c * c + s * s - 1.0L) <= 1e-15L, "c %g s %g", r.c, r.s);      // c: 1.5 eps, s: 2.5 eps, squared and summed: 8 eps
    CHECK(fabs(r.t) <= 1.0, "t %g", r.t);
    if (apq == 0.0) { CHECK(r.c == 1.0 && r.s == 0.0 && r.t == 0.0, "identity"); return; }
    // J' M J with J = [[c, s], [-s, c]]: off-diagonal (c^2 - s^2) apq + c s (app - aqq); first diagonal c^2 app - 2 c s apq + s^2 aqq
    const long double off = (c * c - s * s) * apq + c * s * ((long double)app - aqq);
    CHECK(fabsl(off) <= 8e-16L * sc, "off %Lg scale %Lg (app %g aqq %g apq %g)", off, sc, app, aqq, apq);
    const long double dpp = c * c * app - 2.0L * c * s * apq + s * s * aqq, dqq = s * s * app + 2.0L * c * s * apq + c * c * aqq;
    CHECK(fabsl(dpp - ((long double)app - t * apq)) <= 8e-16L * sc, "a_pp' %Lg", dpp);
    CHECK(fabsl(dqq - ((long double)aqq + t * apq)) <= 8e-16L * sc, "a_qq' %Lg", dqq);
}

static void test_rotation() {
    for (int k = 0; k < 200000; k++) {
        const double e1 = pow(10.0, 12.0 * urand() - 6.0), e2 = pow(10.0, 12.0 * urand() - 6.0), e3 = pow(10.0, 24.0 * urand() - 18.0);
        check_rotation(e1 * nrand(), e2 * nrand(), e3 * nrand());
    }
    check_rotation(1.0, 2.0, 0.0);
    check_rotation(0.0, 0.0, 0.0);
    for (double v : {1.0, -3.5, 0.0, 1e200, 1e-200}) {
        check_rotation(v, v, 0.7);      // equal diagonal entries: theta = 0, t = 1
        CHECK(jacobi_rotation(v, v, 0.7).t == 1.0, "t at theta = 0");
        CHECK(jacobi_rotation(v, v, -0.7).t == 1.0, "t at theta = 0 (sign of theta is that of +0)");
    }
    const JacobiRot h = jacobi_rotation(-1e200, 1e200, 1e-200);      // theta^2 overflows
    CHECK(h.t == 0.0 && h.c == 1.0 && h.s == 0.0, "huge theta: t %g", h.t);
    check_rotation(1.0, 1.0 + 1e-15, 1e-300);
    check_rotation(5e-324, 0.0, 5e-324);
}

static void test_round_robin() {
    for (int n2 = 2; n2 <= 64; n2 += 2) {
        std::vector<int> seen(n2 * n2, 0);
        for (int round = 0; round < n2 - 1; round++) {
            std::vector<int> used(n2, 0);
            for (int slot = 0; slot < n2 / 2; slot++) {
                int p = -1, q = -1;
                round_robin_pair(n2, round, slot, &p, &q);
                CHECK(0 <= p && p < q && q < n2, "n2 %d round %d slot %d: (%d, %d)", n2, round, slot, p, q);
                CHECK(!used[p] && !used[q], "n2 %d round %d: a coordinate in two pairs", n2, round);
                used[p] = used[q] = 1;
                seen[p * n2 + q]++;
            }
        }
        for (int p = 0; p < n2; p++)
            for (int q = p + 1; q < n2; q++) CHECK(seen[p * n2 + q] == 1, "n2 %d: pair (%d, %d) visited %d times", n2, p, q, seen[p * n2 + q]);
    }
}

static void test_tree_sum() {
    double v[64];
    for (int k = 0; k < 64; k++) v[k] = nrand() * pow(10.0, 8.0 * urand());
    double e[8];
    for (int o = 0; o < 8; o++) {
        const double *w = v + 8 * o;
        e[o] = ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
    }
    const double want = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    CHECK(tree_sum64(v) == want, "tree %a want %a", tree_sum64(v), want);
}

// the sweeps of jacobi_small.h, serially: rows, then columns, then the exact entries, slot after slot
static int host_jacobi(std::vector<double> &A, std::vector<double> &Q, int n2, int max_sweeps, double tol) {
    for (int i = 0; i < n2; i++) for (int j = 0; j < n2; j++) Q[i * n2 + j] = i == j;
    double fro2 = 0.0;
    for (int e = 0; e < n2 * n2; e++) fro2 += A[e] * A[e];
    for (int sweeps = 0;; sweeps++) {
        double off2 = 0.0;
        for (int i = 0; i < n2; i++) for (int j = 0; j < n2; j++) if (i != j) off2 += A[i * n2 + j] * A[i * n2 + j];
        if (off2 <= tol * tol * fro2) return sweeps;
        if (sweeps >= max_sweeps) return -1;
        for (int round = 0; round < n2 - 1; round++) {
            std::vector<JacobiRot> rot(n2 / 2);
            std::vector<int> P(n2 / 2), Qi(n2 / 2);
            std::vector<double> app(n2 / 2), aqq(n2 / 2), apq(n2 / 2);
            for (int k = 0; k < n2 / 2; k++) {
                round_robin_pair(n2, round, k, &P[k], &Qi[k]);
                app[k] = A[P[k] * n2 + P[k]]; aqq[k] = A[Qi[k] * n2 + Qi[k]]; apq[k] = A[P[k] * n2 + Qi[k]];
                const JacobiRot id = {1.0, 0.0, 0.0};      // (a negligible a_pq is not rotated: JACOBI_NEGLIGIBLE2 of jacobi_small.h)
                rot[k] = apq[k] * apq[k] <= 0x1p-120 * (tol * tol * fro2) ? id : jacobi_rotation(app[k], aqq[k], apq[k]);
            }
            for (int k = 0; k < n2 / 2; k++) {
                const double c = rot[k].c, s = rot[k].s;
                if (s == 0.0) continue;
                for (int j = 0; j < n2; j++) {
                    double *ap = &A[P[k] * n2 + j], *aq = &A[Qi[k] * n2 + j], *vp = &Q[P[k] * n2 + j], *vq = &Q[Qi[k] * n2 + j];
                    const double a = *ap, b = *aq, u = *vp, v = *vq;
                    *ap = c * a - s * b; *aq = s * a + c * b; *vp = c * u - s * v; *vq = s * u + c * v;
                }
            }
            for (int k = 0; k < n2 / 2; k++) {
                const double c = rot[k].c, s = rot[k].s;
                if (s == 0.0) continue;
                for (int i = 0; i < n2; i++) {
                    double *ap = &A[i * n2 + P[k]], *aq = &A[i * n2 + Qi[k]];
                    const double a = *ap, b = *aq;
                    *ap = c * a - s * b; *aq = s * a + c * b;
                }
            }
            for (int k = 0; k < n2 / 2; k++) {
                if (rot[k].s == 0.0) continue;
                A[P[k] * n2 + P[k]] = app[k] - rot[k].t * apq[k];
                A[Qi[k] * n2 + Qi[k]] = aqq[k] + rot[k].t * apq[k];
                A[P[k] * n2 + Qi[k]] = A[Qi[k] * n2 + P[k]] = 0.0;
            }
        }
    }
}

static void check_jacobi(const std::vector<double> &A0, int n2, const char *what) {
    std::vector<double> A(A0), Q(n2 * n2);
    const int sweeps = host_jacobi(A, Q, n2, 30, 1e-15);
    CHECK(sweeps >= 0 && sweeps <= 12, "%s n2 %d: sweeps %d", what, n2, sweeps);
    long double fro = 0.0L, tr0 = 0.0L, tr1 = 0.0L;
    for (int i = 0; i < n2; i++) { tr0 += A0[i * n2 + i]; tr1 += A[i * n2 + i]; for (int j = 0; j < n2; j++) fro += (long double)A0[i * n2 + j] * A0[i * n2 + j]; }
    fro = sqrtl(fro);
    const long double tol = 1e-13L * (fro > 0.0L ? fro : 1.0L);      // n eps |A|_F = 7e-15 |A|_F at n = 64, with margin
    CHECK(fabsl(tr0 - tr1) <= tol, "%s n2 %d: trace moved by %Lg", what, n2, tr0 - tr1);
    for (int k = 0; k < n2; k++) {
        long double nrm = 0.0L;
        for (int i = 0; i < n2; i++) nrm += (long double)Q[k * n2 + i] * Q[k * n2 + i];
        CHECK(fabsl(nrm - 1.0L) <= 1e-13L, "%s n2 %d: |q_%d|^2 - 1 = %Lg", what, n2, k, nrm - 1.0L);
        for (int i = 0; i < n2; i++) {      // (A0 q_k)_i = lam_k q_k,i
            long double r = 0.0L;
            for (int j = 0; j < n2; j++) r += (long double)A0[i * n2 + j] * Q[k * n2 + j];
            r -= (long double)A[k * n2 + k] * Q[k * n2 + i];
            CHECK(fabsl(r) <= tol, "%s n2 %d: residual %Lg of eigenpair %d at %d", what, n2, r, k, i);
        }
    }
}

static void test_jacobi() {
    for (int n2 : {2, 4, 16, 32, 64}) {
        std::vector<double> A(n2 * n2);
        for (int i = 0; i < n2; i++) for (int j = 0; j <= i; j++) A[i * n2 + j] = A[j * n2 + i] = nrand();
        check_jacobi(A, n2, "random");
        std::vector<double> I(n2 * n2, 0.0);
        for (int i = 0; i < n2; i++) I[i * n2 + i] = 1.0;
        check_jacobi(I, n2, "identity");
        std::vector<double> E(A);      // equal diagonal entries
        for (int i = 0; i < n2; i++) E[i * n2 + i] = 0.5;
        check_jacobi(E, n2, "equal diagonal");
        // a repeated lowest eigenvalue: V diag(-1, -1, rest) V' from the random matrix's own eigenvectors
        std::vector<double> D(A), Q(n2 * n2), R(n2 * n2, 0.0);
        host_jacobi(D, Q, n2, 30, 1e-15);
        for (int k = 0; k < n2; k++) {
            const double lam = k < 2 ? -1.0 : 1.0 + 0.1 * k;
            for (int i = 0; i < n2; i++) for (int j = 0; j < n2; j++) R[i * n2 + j] += lam * Q[k * n2 + i] * Q[k * n2 + j];
        }
        for (int i = 0; i < n2; i++) for (int j = 0; j < i; j++) R[i * n2 + j] = R[j * n2 + i];
        check_jacobi(R, n2, "repeated lowest");
    }
    std::vector<double> pad = {2.0, 0.0, 0.0, 0.0};      // n = 1 padded with a decoupled coordinate: nothing rotates
    std::vector<double> Q(4);
    CHECK(host_jacobi(pad, Q, 2, 30, 1e-15) == 0 && pad[0] == 2.0 && pad[3] == 0.0, "padding");
}

static long double psi_ld(int n, const double *gh, const double *d, double sigma) {
    long double p = 0.0L;
    for (int k = 0; k < n; k++) if (gh[k] != 0.0) { const long double w = (long double)gh[k] / ((long double)d[k] + sigma); p += w * w; }
    return p;
}

static void check_secular(int n, const double *gh, const double *d, double rho, double sigma_lo, const char *what) {
    const SecularRoot r = secular_solve(n, gh, d, rho, sigma_lo);
    CHECK(r.sigma >= sigma_lo && std::isfinite(r.sigma), "%s: sigma %g", what, r.sigma);
    CHECK(r.iters < SECULAR_MAX_ITERS, "%s: %d evaluations", what, r.iters);
    const long double y = sqrtl(psi_ld(n, gh, d, r.sigma));
    // the stop rule is 4 eps on sqrt(psi) as summed in double; the tree sum of 64 terms adds at most 6 eps, each term 3 eps
    CHECK(fabsl(y - rho) <= 1e-14L * rho, "%s: |y| - rho = %Lg (rho %g, sigma %g, %d evaluations)", what, y - rho, rho, r.sigma, r.iters);
}

static void test_secular() {
    double gh[64], d[64];
    for (int rep = 0; rep < 20000; rep++) {
        const int n = 1 + (int)(urand() * 64.0) % 64;
        for (int k = 0; k < n; k++) { gh[k] = nrand(); d[k] = k == 0 ? 0.0 : 10.0 * urand(); }
        if (rep % 3 == 0) for (int k = 1; k < n; k += 2) gh[k] = 0.0;             // zeros in gh
        if (rep % 5 == 0 && n > 2) d[1] = d[2] = 0.0;                             // a repeated lowest eigenvalue
        if (rep % 7 == 0) gh[0] *= pow(10.0, -12.0 * urand());                    // nearly hard: the root far below the spectrum
        const double rho = pow(10.0, 4.0 * urand() - 2.0);
        if (psi_ld(n, gh, d, 0.0) > (long double)rho * rho || gh[0] != 0.0) check_secular(n, gh, d, rho, 0.0, "random");
        // a lower end that is not 0 (the ball with a convex objective, minimiser outside): the root must lie right of it
        const double lo = 0.5 * urand();
        if (psi_ld(n, gh, d, lo) > (long double)rho * rho) check_secular(n, gh, d, rho, lo, "lower end");
    }
    // the rule: gh = 0 on the lowest eigenspace and the rest short -> hard (1); the rest long -> regular; a component above the
    // threshold -> regular; below it -> hard; nothing in L to drop but psi_0 <= rho^2 -> hard (2)
    CHECK(spectral_hard_case(0.0, 0.0, 0.0, 0.0, 1.0) == 1, "g = 0");
    CHECK(spectral_hard_case(0.0, 4.0, 0.5, 0.5, 1.0) == 1, "orthogonal, short");
    CHECK(spectral_hard_case(0.0, 4.0, 1.5, 1.5, 1.0) == 0, "orthogonal, long");
    const double t = SPECTRAL_HARD_THR;
    CHECK(spectral_hard_case(0.99 * t * t * 4.0, 4.0, 0.5, INFINITY, 1.0) == 1, "below the threshold");
    CHECK(spectral_hard_case(1.01 * t * t * 4.0, 4.0, 0.5, INFINITY, 1.0) == 0, "above the threshold");
    CHECK(spectral_hard_case(1.01 * t * t * 4.0, 4.0, 0.5, 0.9, 1.0) == 2, "no root right of 0");
    CHECK(secular_w(0.0, 0.0) == 0.0 && std::isinf(secular_w(1.0, 0.0)), "0 / 0 is 0");
}

int main() {
    test_rotation();
    test_round_robin();
    test_tree_sum();
    test_jacobi();
    test_secular();
    printf("ok %ld\n", checks);
    return 0;
}
