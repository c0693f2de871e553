// The host-compilable pieces of the wide spectral suggest (qcqp_amd/csrc/spectral_solve.h: hestenes_rotation, round_robin_pair up to
// n2 = 128) against long-double references, on random and degenerate inputs.  Built by tests/test_spectral_wide_cpu.py with the host
// compiler, -ffp-contract=off (the device build's setting) and tests/host/hip_stub; prints "ok <checks>" or the first failure.
//   rotation     two columns of m rows, alpha, beta, gamma by fma in ascending row as jacobi_wide.h forms them: below the threshold
//                the identity with s == 0 exactly (gamma == 0, a NaN, tiny columns whose alpha beta underflows); above it c^2 + s^2
//                = 1, and after (g_p, g_q) <- (c g_p - s g_q, s g_p + c g_q) in double the columns are orthogonal and alpha + beta is
//                kept, both in long double to (m + 16) eps (alpha + beta): alpha, beta and gamma carry up to m eps / 2 of
//                |g_p| |g_q| each, the rotation itself a few eps per entry; alpha == beta gives t = 1; columns of 1e150 whose
//                alpha beta overflows; ratios |g_p| / |g_q| from 1e-12 to 1e12
//   round robin  for every even n2 <= 128: the pairs of a round are disjoint, p < q, and a sweep visits every pair exactly once
//   solver       the loop of jacobi_wide.h restated on the host from the two pieces (shift 2 |A|_F, stop after the first sweep without
//                a rotation, normalised columns, Rayleigh quotients): U'U = I and A u_k = lam_k u_k in long double; random matrices of
//                odd and even order, the identity (fully degenerate), a repeated lowest eigenvalue, rank one, the zero matrix; the
//                padding coordinate of an odd order stays put, exactly
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

static const double TOL = 1e-15;
static const long double EPS = 2.220446049250313e-16L;

struct Dots { double alpha, beta, gamma; };
static Dots dots(const std::vector<double> &gp, const std::vector<double> &gq) {
    Dots d = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < gp.size(); i++) {
        d.alpha = fma(gp[i], gp[i], d.alpha);
        d.beta = fma(gq[i], gq[i], d.beta);
        d.gamma = fma(gp[i], gq[i], d.gamma);
    }
    return d;
}

// returns whether the pair was rotated
static bool check_pair(std::vector<double> gp, std::vector<double> gq) {
    const size_t m = gp.size();
    const Dots d = dots(gp, gq);
    const JacobiRot r = hestenes_rotation(d.alpha, d.beta, d.gamma, TOL);
    long double a0 = 0, b0 = 0;
    for (size_t i = 0; i < m; i++) { a0 += (long double)gp[i] * gp[i]; b0 += (long double)gq[i] * gq[i]; }
    if (!(fabs(d.gamma) > TOL * (sqrt(d.alpha) * sqrt(d.beta)))) {
        CHECK(r.c == 1.0 && r.s == 0.0 && r.t == 0.0, "below the threshold: c %g s %g (alpha %g beta %g gamma %g)", r.c, r.s, d.alpha, d.beta, d.gamma);
        return false;
    }
    const long double c = r.c, s = r.s;
    CHECK(std::isfinite(r.c) && std::isfinite(r.s), "alpha %g beta %g gamma %g", d.alpha, d.beta, d.gamma);
    CHECK(fabsl(c * c + s * s - 1.0L) <= 1e-15L, "c %g s %g", r.c, r.s);
    CHECK(fabs(r.t) <= 1.0, "t %g", r.t);
    for (size_t i = 0; i < m; i++) {
        const double a = gp[i], b = gq[i];
        gp[i] = r.c * a - r.s * b;
        gq[i] = r.s * a + r.c * b;
    }
    long double a1 = 0, b1 = 0, g1 = 0;
    for (size_t i = 0; i < m; i++) { a1 += (long double)gp[i] * gp[i]; b1 += (long double)gq[i] * gq[i]; g1 += (long double)gp[i] * gq[i]; }
    const long double bound = (long double)(m + 16) * EPS * (a0 + b0);
    CHECK(fabsl(g1) <= bound, "columns not orthogonal: %Lg against %Lg (alpha %g beta %g gamma %g)", g1, bound, d.alpha, d.beta, d.gamma);
    CHECK(fabsl((a1 + b1) - (a0 + b0)) <= bound, "alpha + beta not kept: %Lg against %Lg", (a1 + b1) - (a0 + b0), bound);
    return true;
}

static void test_rotation() {
    for (int k = 0; k < 40000; k++) {
        const size_t m = 2 + (size_t)(urand() * 127.0);
        const double e1 = pow(10.0, 12.0 * urand() - 6.0), e2 = pow(10.0, 12.0 * urand() - 6.0), mix = k % 3 ? pow(10.0, -16.0 * urand()) : 1.0;
        std::vector<double> gp(m), gq(m);
        for (size_t i = 0; i < m; i++) { gp[i] = e1 * nrand(); gq[i] = e2 * (nrand() + (k % 2 ? mix * gp[i] / e1 : 0.0)); }
        check_pair(gp, gq);
    }
    // gamma == 0 exactly: disjoint supports; and the padding coordinate c e_n against any column with a zero in that row
    CHECK(!check_pair({1.0, 2.0, 0.0, 0.0}, {0.0, 0.0, -3.0, 0.5}), "gamma == 0");
    CHECK(!check_pair({0.3, -0.7, 0.0}, {0.0, 0.0, 12.5}), "the padding coordinate");
    CHECK(!check_pair({0.0, 0.0}, {0.0, 0.0}), "two zero columns");
    const JacobiRot zero = hestenes_rotation(1.0, 1.0, 0.0, 0.0);      // tol = 0 still skips gamma == 0
    CHECK(zero.c == 1.0 && zero.s == 0.0, "gamma == 0 at tol == 0");
    // alpha == beta: theta == 0, t = 1, c = s = 1 / sqrt(2) up to the sign of gamma
    for (double g : {0.5, -0.5, 1e-9}) {
        const JacobiRot r = hestenes_rotation(2.0, 2.0, g, TOL);
        CHECK(r.t == 1.0 && r.c == r.s && fabs(r.c - 0.7071067811865476) <= 2.3e-16, "alpha == beta: t %g c %g s %g", r.t, r.c, r.s);
    }
    CHECK(check_pair({1.0, 2.0}, {2.0, 1.0}), "alpha == beta in columns");
    // huge columns: alpha beta overflows, its root taken factor by factor does not
    CHECK(check_pair({1e150, 1e150}, {1e150, 0.0}), "huge columns must rotate");
    const JacobiRot hr = hestenes_rotation(2e300, 1e300, 1e300, TOL);
    CHECK(hr.s != 0.0 && std::isfinite(hr.c) && std::isfinite(hr.s), "huge: c %g s %g", hr.c, hr.s);
    // tiny columns that are orthogonal to the threshold: alpha beta underflows to 0, and a threshold of 0 would rotate them
    CHECK(!check_pair({1e-150, 0.0}, {1e-166, 1e-150}), "tiny columns below the threshold");
    CHECK(check_pair({1e-150, 1e-150}, {1e-150, 0.0}), "tiny columns must rotate");
    // huge and tiny ratios of the two norms
    for (double ratio : {1e-12, 1e-6, 1e6, 1e12}) {
        CHECK(check_pair({1.0, 1.0, 0.5}, {ratio, 0.0, -0.25 * ratio}), "ratio %g", ratio);
        CHECK(check_pair({ratio, ratio}, {1.0, 0.0}), "ratio %g", ratio);
    }
    // a NaN among the three: not rotated
    const double nan = std::nan("");
    for (int k = 0; k < 3; k++) {
        const JacobiRot r = hestenes_rotation(k == 0 ? nan : 1.0, k == 1 ? nan : 1.0, k == 2 ? nan : 0.5, TOL);
        CHECK(r.c == 1.0 && r.s == 0.0, "NaN in argument %d", k);
    }
}

static void test_round_robin() {
    for (int n2 = 2; n2 <= 128; n2 += 2) {
        std::vector<int> seen(n2 * n2, 0);
        for (int round = 0; round < n2 - 1; round++) {
            std::vector<int> used(n2, 0);
            for (int slot = 0; slot < n2 / 2; slot++) {
                int p = -1, q = -1;
                round_robin_pair(n2, round, slot, &p, &q);
                CHECK(0 <= p && p < q && q < n2, "n2 %d round %d slot %d: (%d, %d)", n2, round, slot, p, q);
                CHECK(!used[p] && !used[q], "n2 %d round %d: a column twice", n2, round);
                used[p] = used[q] = 1;
                seen[p * n2 + q]++;
            }
        }
        for (int p = 0; p < n2; p++)
            for (int q = p + 1; q < n2; q++) CHECK(seen[p * n2 + q] == 1, "n2 %d: pair (%d, %d) %d times", n2, p, q, seen[p * n2 + q]);
    }
}

// jacobi_wide.h on the host: G column-major with stride n2 (one lane after the other; the pairs of a round own disjoint columns).
// Returns the sweeps, -1 if max_sweeps ran out.
static int solve(const std::vector<double> &A, int n, std::vector<double> &U, std::vector<double> &lam) {
    const int n2 = (n + 1) & ~1;
    std::vector<double> G((size_t)n2 * n2, 0.0);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) G[(size_t)j * n2 + i] = A[(size_t)i * n + j];
    double fro2 = 0.0;
    for (double v : G) fro2 += v * v;
    U.assign((size_t)n2 * n2, 0.0);
    lam.assign(n2, 0.0);
    if (fro2 == 0.0) { for (int k = 0; k < n2; k++) U[(size_t)k * n2 + k] = 1.0; return 0; }
    const double c = 2.0 * sqrt(fro2);
    for (int k = 0; k < n2; k++) G[(size_t)k * n2 + k] += c;
    int sweeps = 0;
    bool converged = false;
    while (sweeps < 30 && !converged) {
        bool rotated = false;
        for (int round = 0; round < n2 - 1; round++)
            for (int slot = 0; slot < n2 / 2; slot++) {
                int p, q;
                round_robin_pair(n2, round, slot, &p, &q);
                double *gp = &G[(size_t)p * n2], *gq = &G[(size_t)q * n2];
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = 0; i < n2; i++) { alpha = fma(gp[i], gp[i], alpha); beta = fma(gq[i], gq[i], beta); gamma = fma(gp[i], gq[i], gamma); }
                const JacobiRot r = hestenes_rotation(alpha, beta, gamma, TOL);
                if (r.s == 0.0) continue;
                rotated = true;
                for (int i = 0; i < n2; i++) { const double a = gp[i], b = gq[i]; gp[i] = r.c * a - r.s * b; gq[i] = r.s * a + r.c * b; }
            }
        sweeps++;
        converged = !rotated;
    }
    for (int k = 0; k < n2; k++) {
        double nn = 0.0;
        for (int i = 0; i < n2; i++) nn = fma(G[(size_t)k * n2 + i], G[(size_t)k * n2 + i], nn);
        for (int i = 0; i < n2; i++) U[(size_t)k * n2 + i] = G[(size_t)k * n2 + i] / sqrt(nn);
    }
    for (int k = 0; k < n; k++) {
        double l = 0.0;
        for (int i = 0; i < n; i++) {
            double t = 0.0;
            for (int j = 0; j < n; j++) t = fma(A[(size_t)i * n + j], U[(size_t)k * n2 + j], t);
            l = fma(U[(size_t)k * n2 + i], t, l);
        }
        lam[k] = l;
    }
    return converged ? sweeps : -1;
}

static void check_solve(const std::vector<double> &A, int n, const char *what) {
    const int n2 = (n + 1) & ~1;
    std::vector<double> U, lam;
    const int sweeps = solve(A, n, U, lam);
    long double fro = 0;
    for (double v : A) fro += (long double)v * v;
    fro = sqrtl(fro);
    CHECK(sweeps >= 0 && sweeps <= 16, "%s n %d: %d sweeps", what, n, sweeps);
    if (fro == 0) CHECK(sweeps == 0, "%s: a sweep on the zero matrix", what);
    for (int k = 0; k < n2; k++)
        for (int l = k; l < n2; l++) {
            long double d = 0;
            for (int i = 0; i < n2; i++) d += (long double)U[(size_t)k * n2 + i] * U[(size_t)l * n2 + i];
            CHECK(fabsl(d - (k == l ? 1.0L : 0.0L)) <= 1e-14L, "%s n %d: u_%d . u_%d = %Lg", what, n, k, l, d);
        }
    for (int k = 0; k < n; k++)
        for (int i = 0; i < n; i++) {
            long double au = 0;
            for (int j = 0; j < n; j++) au += (long double)A[(size_t)i * n + j] * U[(size_t)k * n2 + j];
            // |A u - lam u| <= (angle between u_k and the eigenspace, some n eps times the condition 3 of G) x the spread 2 |A|_F
            CHECK(fabsl(au - (long double)lam[k] * U[(size_t)k * n2 + i]) <= 1e-13L * fro, "%s n %d: (A u - lam u)_%d of vector %d = %Lg, |A|_F %Lg", what, n, i, k,
                  au - (long double)lam[k] * U[(size_t)k * n2 + i], fro);
        }
    if (n2 != n)       // the padding coordinate: column n is e_n and row n of every other column is 0, exactly
        for (int k = 0; k < n2; k++) {
            CHECK(U[(size_t)n * n2 + k] == (k == n ? 1.0 : 0.0), "%s n %d: the padding column moved at row %d", what, n, k);
            CHECK(U[(size_t)k * n2 + n] == (k == n ? 1.0 : 0.0), "%s n %d: the padding row moved at column %d", what, n, k);
        }
}

static void test_solver() {
    for (int n : {1, 2, 3, 6, 17, 40, 65}) {
        std::vector<double> A((size_t)n * n), Z((size_t)n * n, 0.0), I((size_t)n * n, 0.0), R((size_t)n * n), D((size_t)n * n, 0.0);
        std::vector<double> v(n);
        for (int i = 0; i < n; i++) {
            v[i] = nrand();
            I[(size_t)i * n + i] = 1.0;
            D[(size_t)i * n + i] = i < 3 ? -2.0 : 1.0 + i;       // a lowest eigenvalue of multiplicity three (up to n = 3: a multiple of I)
            for (int j = 0; j <= i; j++) A[(size_t)i * n + j] = A[(size_t)j * n + i] = nrand();
        }
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) R[(size_t)i * n + j] = v[i] * v[j];
        check_solve(A, n, "random");
        check_solve(Z, n, "zero");
        check_solve(I, n, "identity");
        check_solve(R, n, "rank one");
        // the repeated eigenvalue in a rotated basis: H D H with the reflector H = I - 2 v v' / v'v
        std::vector<double> H((size_t)n * n), HD((size_t)n * n, 0.0), M((size_t)n * n, 0.0);
        double vv = 0.0;
        for (int i = 0; i < n; i++) vv += v[i] * v[i];
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) H[(size_t)i * n + j] = (i == j ? 1.0 : 0.0) - 2.0 * v[i] * v[j] / vv;
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) HD[(size_t)i * n + j] = H[(size_t)i * n + j] * D[(size_t)j * n + j];
        for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) {
            double t = 0.0;
            for (int k = 0; k < n; k++) t += HD[(size_t)i * n + k] * H[(size_t)j * n + k];
            M[(size_t)i * n + j] = M[(size_t)j * n + i] = t;
        }
        check_solve(M, n, "repeated lowest eigenvalue");
    }
}

int main() {
    test_rotation();
    test_round_robin();
    test_solver();
    printf("ok %ld\n", checks);
    return 0;
}
