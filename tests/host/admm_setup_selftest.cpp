// The scalar pieces of the device-side ADMM setup (qcqp_amd/csrc/admm_setup_rule.h) on the host.  Built by
// tests/test_admm_setup_cpu.py with the host compiler, -ffp-contract=off (the device build's setting) and tests/host/hip_stub; prints
// "ok <checks>" or the first failure.
//   rule      admm_setup_rho against the rule written out step by step in double (the bits of qcqp_amd.batch.admm_rhos) and against a
//             long-double evaluation (2 eps); the branch at lambda_min = 0: +0.0, -0.0 and a NaN take 50 / m, the smallest negative
//             number takes the other branch; the jump there is a factor of two
//   given     admm_setup_rho_too_small is lambda_min + m rho < 0 with the product formed first; exactly on the threshold: not too small
//   weight    admm_setup_weight against long double (2 eps) and positive wherever the given-rho test passes with a margin; with it
//             sum_k w_k u_k u_k' inverts 2 (P0 + rho m I) on a 2 x 2 example to 16 eps (condition 1.02; lam, u and w a few eps each)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "admm_setup_rule.h"

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

static const long double EPS = 2.220446049250313e-16L;

static void test_rule() {
    for (int k = 0; k < 200000; k++) {
        const double m = 1.0 + floor(urand() * 300.0);
        const double lmin = (urand() - 0.5) * pow(10.0, 8.0 * urand() - 4.0);
        const double got = admm_setup_rho(lmin, m);
        volatile double a = 1.0 - lmin, b = 2.0 * a, c = b / m, d = 1.0 / m;      // one rounding per step
        const double want = lmin < 0.0 ? 50.0 * c : 50.0 * d;
        CHECK(got == want, "lmin %g m %g: %.17g against %.17g", lmin, m, got, want);
        const long double ref = lmin < 0.0 ? 100.0L * (1.0L - (long double)lmin) / m : 50.0L / m;
        CHECK(fabsl(got - ref) <= 2.0L * EPS * ref, "lmin %g m %g: %.17g against %.17Lg", lmin, m, got, ref);
        CHECK(got > 0.0 && std::isfinite(got), "lmin %g m %g: %g", lmin, m, got);
    }
    for (double m : {1.0, 3.0, 192.0}) {
        const double flat = 50.0 * (1.0 / m);
        CHECK(admm_setup_rho(0.0, m) == flat && admm_setup_rho(-0.0, m) == flat, "zero at m %g", m);
        CHECK(admm_setup_rho(std::nan(""), m) == flat, "NaN at m %g", m);
        CHECK(admm_setup_rho(5e-324, m) == flat, "the smallest positive number at m %g", m);
        const double below = admm_setup_rho(-5e-324, m);
        CHECK(below == 50.0 * (2.0 / m) && fabs(below / flat - 2.0) <= 1e-15, "the jump at m %g: %g against %g", m, below, flat);
    }
}

static void test_given() {
    for (int k = 0; k < 200000; k++) {
        const double m = 1.0 + floor(urand() * 300.0), rho = pow(10.0, 6.0 * urand() - 3.0);
        const double lmin = -(m * rho) * (0.5 + urand());
        volatile double prod = m * rho, sum = lmin + prod;
        CHECK(admm_setup_rho_too_small(lmin, m, rho) == (sum < 0.0), "lmin %g m %g rho %g", lmin, m, rho);
        CHECK(!admm_setup_rho_too_small(-prod, m, rho), "on the threshold: lmin %g m %g rho %g", -prod, m, rho);
        CHECK(!admm_setup_rho_too_small(fabs(lmin), m, rho), "a positive lambda_min");
    }
    CHECK(!admm_setup_rho_too_small(std::nan(""), 4.0, 1.0), "a NaN is left to the status of the decomposition");
}

static void test_weight() {
    for (int k = 0; k < 200000; k++) {
        const double m = 1.0 + floor(urand() * 300.0), rho = pow(10.0, 6.0 * urand() - 3.0);
        const double lam = (m * rho) * (4.0 * urand() - 0.99);       // lam + rho m >= 0.01 rho m
        const double w = admm_setup_weight(lam, rho, m);
        const long double ref = 1.0L / (2.0L * ((long double)lam + (long double)rho * m));
        // rho m and the sum round once each: relative eps / 2 of (|lam| + rho m) against the sum, at most 199 times its size here
        const long double cond = (fabsl((long double)lam) + (long double)rho * m) / ((long double)lam + (long double)rho * m);
        CHECK(w > 0.0 && fabsl(w - ref) <= (2.0L + 2.0L * cond) * EPS * ref, "lam %g rho %g m %g: %.17g against %.17Lg", lam, rho, m, w, ref);
    }
    // P0 = [[2, 1], [1, -1]], m = 3, rho by the rule: u u' sums weighted by w invert 2 (P0 + rho m I)
    const double P[2][2] = {{2.0, 1.0}, {1.0, -1.0}}, m = 3.0;
    const double disc = sqrt(13.0), lam[2] = {(1.0 - disc) / 2.0, (1.0 + disc) / 2.0};
    const double rho = admm_setup_rho(lam[0], m);
    double Minv[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int k = 0; k < 2; k++) {
        const double ux = 1.0, uy = lam[k] - 2.0, nrm = sqrt(ux * ux + uy * uy), u[2] = {ux / nrm, uy / nrm};
        const double w = admm_setup_weight(lam[k], rho, m);
        for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) Minv[i][j] = fma(u[i] * u[j], w, Minv[i][j]);
    }
    CHECK(Minv[0][1] == Minv[1][0], "the product of the vector entries first: symmetric bits");
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) {
            long double s = 0;
            for (int k = 0; k < 2; k++) s += 2.0L * ((long double)P[i][k] + (i == k ? (long double)rho * m : 0.0L)) * Minv[k][j];
            CHECK(fabsl(s - (i == j ? 1.0L : 0.0L)) <= 16.0L * EPS, "2 (P0 + rho m I) Minv at (%d, %d): %Lg", i, j, s);
        }
}

int main() {
    test_rule();
    test_given();
    test_weight();
    printf("ok %ld\n", checks);
    return 0;
}
