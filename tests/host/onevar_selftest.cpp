// The one-variable solver's device headers on the host: every variant of csrc/unit_variants.h (the functions the unit operators
// qcqpmi_onevar_variant_batch / qcqpmi_p1_visit_batch run one lane per case) over a case file written by
// tests/test_onevar_lattice_cpu.py, which compares the output with the oracle value by value.
//   onevar_selftest onevar VARIANT in out     in : int64 count, f0[count x 3], fs[count x 4 x 4], s[count], int32 nf[count], uint64 seed
//                                             out: per case 13 doubles: status, x, n, 5 x (lo, hi)
//   onevar_selftest visit VARIANT in out      in : int64 count, cons[count x 4 x 4], xi[count], int32 nf[count], tol, viol_tol, uint64 seed, int64 sweep
//                                             out: per case 4 doubles: x after the visit, moved, vafter, status
// A case outside the variant's contract ends the program with status 3.  Build with -ffp-contract=off, the device build's setting.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "unit_variants.h"

using namespace qcqpmi;

template <typename T>
static void rd(FILE *f, T *p, size_t cnt) {
    if (cnt && fread(p, sizeof(T), cnt, f) != cnt) { fprintf(stderr, "short case file\n"); exit(2); }
}

template <int V>
static void run_onevar(int64_t N, const double *f0, const double *fs, const int *nf, const double *s, uint64_t seed, double *out) {
    std::vector<double> x(N), C(N * 10);
    std::vector<int> st(N), nC(N);
    for (int64_t i = 0; i < N; i++) uv_onevar_case<V>(i, f0, fs, nf, s, seed, x.data(), st.data(), C.data(), nC.data());
    for (int64_t i = 0; i < N; i++) {
        out[13 * i] = st[i]; out[13 * i + 1] = x[i]; out[13 * i + 2] = nC[i];
        memcpy(out + 13 * i + 3, C.data() + 10 * i, 10 * sizeof(double));
    }
}

template <int V>
static void run_visit(int64_t N, const double *cons, const int *nf, const double *xi, double tol, double viol_tol, uint64_t seed,
                      int64_t sweep, double *out) {
    std::vector<double> x(N), va(N);
    std::vector<int> mv(N), st(N);
    for (int64_t i = 0; i < N; i++) pv_visit_case<V>(i, N, cons, nf, xi, tol, viol_tol, seed, sweep, x.data(), mv.data(), va.data(), st.data());
    for (int64_t i = 0; i < N; i++) { out[4 * i] = x[i]; out[4 * i + 1] = mv[i]; out[4 * i + 2] = va[i]; out[4 * i + 3] = st[i]; }
}

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: onevar_selftest onevar|visit VARIANT in out\n"); return 2; }
    const bool visit = !strcmp(argv[1], "visit");
    const int variant = atoi(argv[2]);
    if (variant < 0 || variant >= (visit ? (int)PV_VISIT_VARIANTS : (int)UV_ONEVAR_VARIANTS)) { fprintf(stderr, "unknown variant\n"); return 2; }
    FILE *f = fopen(argv[3], "rb");
    if (!f) { perror(argv[3]); return 2; }
    int64_t N = 0;
    rd(f, &N, 1);
    if (N <= 0) return 2;
    std::vector<double> out;
    if (!visit) {
        std::vector<double> f0(3 * N), fs(16 * N), s(N);
        std::vector<int> nf(N);
        uint64_t seed;
        rd(f, f0.data(), 3 * N); rd(f, fs.data(), 16 * N); rd(f, s.data(), N); rd(f, nf.data(), N); rd(f, &seed, 1);
        for (int64_t i = 0; i < N; i++)
            if (!uv_case_ok(variant, nf[i])) { fprintf(stderr, "case %lld is outside the contract of variant %d\n", (long long)i, variant); return 3; }
        out.assign(13 * N, 0.0);
        switch (variant) {
        case UV_SWEEP4: run_onevar<UV_SWEEP4>(N, f0.data(), fs.data(), nf.data(), s.data(), seed, out.data()); break;
        case UV_SWEEP2: run_onevar<UV_SWEEP2>(N, f0.data(), fs.data(), nf.data(), s.data(), seed, out.data()); break;
        case UV_SWEEP1: run_onevar<UV_SWEEP1>(N, f0.data(), fs.data(), nf.data(), s.data(), seed, out.data()); break;
        case UV_SINGLE4: run_onevar<UV_SINGLE4>(N, f0.data(), fs.data(), nf.data(), s.data(), seed, out.data()); break;
        case UV_SINGLE2: run_onevar<UV_SINGLE2>(N, f0.data(), fs.data(), nf.data(), s.data(), seed, out.data()); break;
        default: run_onevar<UV_SINGLE1>(N, f0.data(), fs.data(), nf.data(), s.data(), seed, out.data()); break;
        }
    } else {
        std::vector<double> cons(16 * N), xi(N);
        std::vector<int> nf(N);
        double tol, viol_tol;
        uint64_t seed;
        int64_t sweep;
        rd(f, cons.data(), 16 * N); rd(f, xi.data(), N); rd(f, nf.data(), N); rd(f, &tol, 1); rd(f, &viol_tol, 1); rd(f, &seed, 1); rd(f, &sweep, 1);
        for (int64_t i = 0; i < N; i++)
            if (!pv_case_ok(variant, cons.data() + 16 * i, nf[i])) { fprintf(stderr, "case %lld is outside the contract of variant %d\n", (long long)i, variant); return 3; }
        out.assign(4 * N, 0.0);
        switch (variant) {
        case PV_CORE1: run_visit<PV_CORE1>(N, cons.data(), nf.data(), xi.data(), tol, viol_tol, seed, sweep, out.data()); break;
        case PV_CORE4: run_visit<PV_CORE4>(N, cons.data(), nf.data(), xi.data(), tol, viol_tol, seed, sweep, out.data()); break;
        case PV_BAND: run_visit<PV_BAND>(N, cons.data(), nf.data(), xi.data(), tol, viol_tol, seed, sweep, out.data()); break;
        case PV_BAND_N2: run_visit<PV_BAND_N2>(N, cons.data(), nf.data(), xi.data(), tol, viol_tol, seed, sweep, out.data()); break;
        default: run_visit<PV_BAND_N2_FASTA>(N, cons.data(), nf.data(), xi.data(), tol, viol_tol, seed, sweep, out.data()); break;
        }
    }
    fclose(f);
    f = fopen(argv[4], "wb");
    if (!f) { perror(argv[4]); return 2; }
    if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
