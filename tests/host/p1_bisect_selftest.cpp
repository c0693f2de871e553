// qcqp_amd/csrc/p1_bisect.h on the host: the bisection as the kernels run it (phase A + general loop, p1_band_bisect<2>) against the
// general loop alone (p1_band_bisect_general<2>), every field of the final state bit for bit.  Build with -ffp-contract=off.
// Prints "ok <visits compared>" or the first mismatches.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "p1_bisect.h"

using namespace qcqpmi;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {          // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double next_unit() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

static long compared = 0, bad = 0;

struct State {
    double ss[2], es[2], sp[2];
    uint32_t it[2], itp[2];
    bool pending[2];
};

static void init(State &S, double tol, const double (&es)[2]) {
    for (int k = 0; k < 2; k++) { S.ss[k] = -tol; S.es[k] = es[k]; S.sp[k] = 0.0; S.it[k] = 0; S.itp[k] = 0; S.pending[k] = false; }
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// one fused pair: es as the visit would set it (viol - viol_tol, or -tol for a padding element)
static void check_pair(double p, double r, double tol, const double (&es)[2]) {
    State A, B;
    init(A, tol, es);
    init(B, tol, es);
    p1_band_bisect<2>(p, r, tol, A.ss, A.es, A.sp, A.it, A.itp, A.pending);
    p1_band_bisect_general<2>(p, r, tol, 1e-9 * (1.0 - r), B.ss, B.es, B.sp, B.it, B.itp, B.pending);
    for (int k = 0; k < 2; k++) {
        compared++;
        const bool ok = same_bits(A.ss[k], B.ss[k]) && same_bits(A.es[k], B.es[k]) && same_bits(A.sp[k], B.sp[k]) && A.it[k] == B.it[k] &&
                        A.itp[k] == B.itp[k] && A.pending[k] == B.pending[k];
        if (!ok && bad++ < 10)
            std::printf("MISMATCH p=%g r=%g tol=%g es0=%.17g: fast ss=%.17g es=%.17g sp=%.17g it=%u itp=%u pend=%d | general ss=%.17g es=%.17g "
                        "sp=%.17g it=%u itp=%u pend=%d\n", p, r, tol, es[k], A.ss[k], A.es[k], A.sp[k], A.it[k], A.itp[k], (int)A.pending[k],
                        B.ss[k], B.es[k], B.sp[k], B.it[k], B.itp[k], (int)B.pending[k]);
    }
}

int main() {
#if !QCQPMI_P1_FASTBISECT
    std::printf("built without the fast phase: nothing to compare\n");
    return 2;
#endif
    const double tols[2][2] = {{1e-4, 1e-2}, {1e-6, 1e-3}};       // (tol, viol_tol): the defaults and a tighter pair
    const double rs[2] = {-1.0, -4.0};
    const long per_combo = 1250000;       // pairs: 2 x 1.25e6 visits x 4 combinations = 1e7 random violations
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const double tol = tols[a][0], viol_tol = tols[a][1], r = rs[b], p = (b == 0) ? 1.0 : 0.25;
            const double guard = 1e-9 * (1.0 - r);
            // random violations in [0, 1e9]: log-uniform (1e-12 .. 1e9) and uniform, paired at random so that the fused trip counts differ
            for (long i = 0; i < per_combo; i++) {
                double es[2];
                for (int k = 0; k < 2; k++) {
                    const double viol = (next_u64() & 1) ? std::pow(10.0, -12.0 + 21.0 * next_unit()) : 1e9 * next_unit();
                    es[k] = viol - viol_tol;
                }
                if ((i & 1023) == 0) es[1] = -tol;      // a padding element now and then
                check_pair(p, r, tol, es);
            }
            // edge values of viol - viol_tol
            std::vector<double> edge;
            const double base[] = {-viol_tol, -viol_tol / 2.0, -tol, -1e-300, -0.0, 0.0, 4.9e-324, 1e-300, tol / 2.0, tol, 2.0 * tol, 3.0 * tol,
                                   1.0, 1e9, 1e100, 1e300, DBL_MAX / 4.0, DBL_MAX, std::nan("")};
            for (double v : base) {
                edge.push_back(v);
                edge.push_back(std::nextafter(v, INFINITY));
                edge.push_back(std::nextafter(v, -INFINITY));
            }
            // violations formed the way the visit forms them (viol - viol_tol), around viol_tol + tol
            for (double d : {0.0, 1e-300, 4e-9, -4e-9, 1e-16, -1e-16}) edge.push_back((viol_tol + tol + d) - viol_tol);
            // midpoint number k + 1 within +- a few guards of 0: es = tol (2^(k+1) - 1) + d, every step before it in phase A
            const double ds[] = {0.0, 0.25, 0.5, 0.999, 1.0, 1.001, 2.0, 4.0, 16.0};
            for (int k = 0; k <= 40; k++)
                for (double d : ds)
                    for (double sg : {1.0, -1.0}) {
                        const double e0 = tol * (std::ldexp(1.0, k + 1) - 1.0) + sg * d * guard * std::ldexp(1.0, k + 1);
                        edge.push_back(e0);
                        edge.push_back(std::nextafter(e0, INFINITY));
                        edge.push_back(std::nextafter(e0, -INFINITY));
                    }
            // (the first midpoint is (es - tol) / 2: es = tol + 2 d guard puts it at d guard)
            for (double d : ds)
                for (double sg : {1.0, -1.0}) edge.push_back(tol + sg * 2.0 * d * guard);
            for (size_t i = 0; i < edge.size(); i++)
                if (std::isinf(edge[i])) edge[i] = DBL_MAX;       // (an infinite violation never ends the reference's loop either)
            for (size_t i = 0; i < edge.size(); i++) {
                const double e1[2] = {edge[i], -tol}, e2[2] = {-tol, edge[i]}, e3[2] = {edge[i], edge[(i * 7 + 3) % edge.size()]};
                check_pair(p, r, tol, e1);
                check_pair(p, r, tol, e2);
                check_pair(p, r, tol, e3);
            }
        }
    if (bad) {
        std::printf("%ld of %ld visits differ\n", bad, compared);
        return 1;
    }
    std::printf("ok %ld\n", compared);
    return 0;
}
