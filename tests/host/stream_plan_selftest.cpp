// stream_plan (qcqp_amd/csrc/cd_life_plan.h) on the host: the decision of a streamed coordinate-descent run -- which kernel, which
// instantiation, which pre-passes, which buffers -- for the named shapes of DESIGN.md section 4.1, and its invariants over a grid of
// sizes and switches.  Plain C++: no HIP, no environment (the switches are passed in).  Prints "ok <plans checked>".
#include <cstdio>
#include <cstring>

#include "cd_life_plan.h"

using namespace qcqpmi;

static long long g_checked = 0;
static int g_failed = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (g_failed++ < 20) printf("line %d: %s\n", __LINE__, #cond);           \
        }                                                                            \
    } while (0)

static const int CUS = 256;

// separable constraints on n coordinates: maxc per coordinate at most, Kreal classes, objclass / symcls as qcqpmi_finalize finds them;
// the round-4 kernel's own rule (one mirrored class on a positive diagonal, n a multiple of 16 up to 1024) as the host states it
static StreamShape shape(int n, int maxc, int Kreal, int objclass, bool symcls) {
    StreamShape s;
    s.NB = (n + 15) / 16; s.sep = true; s.maxc = maxc; s.Kreal = Kreal; s.objclass = objclass; s.symcls = symcls;
    s.queue_ok = maxc == 1 && Kreal == 1 && objclass == 1 && symcls && n % 16 == 0 && n >= 48 && n <= 1024;
    return s;
}
static StreamShape bls(int n) { return shape(n, 1, 1, 1, true); }         // Boolean least squares: x_i^2 == 1, P0 = A^T A
static StreamShape maxcut(int n) { return shape(n, 1, 1, 2, true); }      // x_i^2 == 1, zero diagonal

static StreamSwitches defaults() {
    StreamSwitches w;
    w.life_version = 0; w.force_generic = false; w.dbg = 0; w.lr_RB = 0; w.profile = false;
    w.prebuilt = true; w.y0_max = STREAM_Y0_ALL; w.rot = STREAM_ROT_AUTO; w.tiles = 0;
    return w;
}
static StreamSwitches factor(int columns) { StreamSwitches w = defaults(); w.lr_RB = (columns + 15) / 16; return w; }

static bool named(const StreamPlan &p, const char *name) { return p.supported && strcmp(p.name, name) == 0; }

static void table() {
    // the headline: n = 1024, rank 256, 20 populations of 4096 restarts
    StreamPlan p = stream_plan(bls(1024), factor(256), 20, 4096, CUS);
    CHECK(named(p, "cd_life_kernel<3,band,factored>") && p.kernel == STREAM_LIFE2 && p.nmw == 3 && p.cs == 0 && p.lr && p.factor_rb == 16);
    CHECK(p.pre && p.y0_count == 20 * 4096 && p.tiles == 1 && p.wgs == 2 * CUS && p.rot == 2);
    CHECK(p.l2_scratch == (size_t)2 * CUS * 1024 * 16 && p.l2_preslack == 20 * 4096 && p.l2_y0 == (size_t)(20 * 4096 / 16) * 16 * 256);
    CHECK(p.outputs == 20 * 4096 && p.bestK == 20 && p.life_prof == 0);
    // ... without the factor (qcqpmi_cd_life_version(3)): the chain takes four blocks, no pre-pass
    StreamSwitches w = factor(256);
    w.life_version = 3;
    p = stream_plan(bls(1024), w, 20, 4096, CUS);
    CHECK(named(p, "cd_life_kernel<3,band>") && p.cs == 4 && !p.lr && !p.pre && p.y0_count == 0 && p.l2_preslack == 0 && p.l2_y0 == 0 && p.rot == 0);
    // ... the round-4 kernel (qcqpmi_cd_life_version(1))
    w.life_version = 1;
    p = stream_plan(bls(1024), w, 20, 4096, CUS);
    CHECK(named(p, "cd_phase2_qs_kernel<lifecycle>") && p.kernel == STREAM_ROUND4 && p.cs == 4 && p.wgs == CUS && p.l2_scratch == 0 && !p.pre);
    // MAXCUT n = 2000: seven multiplying waves, one workgroup per CU
    p = stream_plan(maxcut(2000), defaults(), 1, 4096, CUS);
    CHECK(named(p, "cd_life_kernel<7,lin>") && p.nmw == 7 && p.cs == 4 && p.wgs == CUS && p.l2_scratch == (size_t)CUS * 2000 * 16);
    // n = 4096 needs the factor; n = 2320 is past the seven waves' range without one (n = 2304 is the last inside)
    p = stream_plan(bls(4096), factor(256), 1, 64, CUS);
    CHECK(named(p, "cd_life_kernel<3,band,factored>") && p.nmw == 3 && p.cs == 0 && p.wgs == 4);
    p = stream_plan(shape(4096, 1, 1, 1, false), factor(256), 1, 64, CUS);
    CHECK(named(p, "cd_life_kernel<3,gen,factored>"));
    CHECK(!stream_plan(bls(4096), defaults(), 1, 64, CUS).supported);
    CHECK(!stream_plan(bls(2320), defaults(), 1, 64, CUS).supported);
    CHECK(named(stream_plan(bls(2304), defaults(), 1, 64, CUS), "cd_life_kernel<7,band>"));
    CHECK(!stream_plan(bls(4112), factor(256), 1, 64, CUS).supported);
    // three blocks, n a multiple of 16 or not: the chain multiplies nothing
    p = stream_plan(bls(48), defaults(), 2, 20, CUS);
    CHECK(named(p, "cd_life_kernel<3,band>") && bls(48).NB == 3 && p.cs == 0 && p.wgs == 3);
    p = stream_plan(bls(40), defaults(), 2, 20, CUS);
    CHECK(named(p, "cd_life_kernel<3,band>") && bls(40).NB == 3 && p.cs == 0);
    w = defaults(); w.life_version = 1;
    p = stream_plan(bls(48), w, 2, 20, CUS);
    CHECK(named(p, "cd_phase2_qs_kernel<lifecycle>") && p.cs == 0 && p.wgs == 3);
    CHECK(!stream_plan(bls(40), w, 2, 20, CUS).supported);       // (the round-4 kernel wants whole blocks)
    CHECK(named(stream_plan(maxcut(64), defaults(), 2, 20, CUS), "cd_life_kernel<3,lin>"));
    CHECK(!stream_plan(bls(32), defaults(), 2, 20, CUS).supported);
    // the least the factored kernel takes: n = 128 (eight blocks), here with a factor of 16 columns
    p = stream_plan(bls(128), factor(16), 2, 20, CUS);
    CHECK(named(p, "cd_life_kernel<3,band,factored>") && p.pre && p.y0_count == 40 && p.l2_y0 == 3 * 256);
    CHECK(named(stream_plan(bls(112), factor(16), 2, 20, CUS), "cd_life_kernel<3,band>"));
    w = factor(16); w.life_version = 3;
    p = stream_plan(bls(128), w, 2, 20, CUS);
    CHECK(named(p, "cd_life_kernel<3,band>") && p.cs == 4);
    // several classes, two constraints per coordinate
    CHECK(named(stream_plan(shape(64, 2, 4, 1, false), defaults(), 2, 20, CUS), "cd_life_kernel<3,gen,classes>"));
    CHECK(named(stream_plan(shape(64, 2, 4, 2, false), defaults(), 2, 20, CUS), "cd_life_kernel<3,lin,classes>"));
    CHECK(named(stream_plan(shape(64, 2, 4, 1, false), factor(16), 2, 20, CUS), "cd_life_kernel<3,gen,classes>"));
    CHECK(!stream_plan(shape(64, 2, 5, 1, false), defaults(), 2, 20, CUS).supported);
    CHECK(!stream_plan(shape(64, 3, 1, 1, false), defaults(), 2, 20, CUS).supported);
    // a diagonal of mixed sign: one class with one constraint per coordinate only
    CHECK(!stream_plan(shape(64, 1, 2, 0, false), defaults(), 2, 20, CUS).supported);
    CHECK(!stream_plan(shape(64, 2, 1, 0, false), defaults(), 2, 20, CUS).supported);
    CHECK(named(stream_plan(shape(64, 1, 1, 0, false), defaults(), 2, 20, CUS), "cd_life_kernel<3,sgn>"));
    CHECK(named(stream_plan(shape(2000, 1, 1, 0, false), factor(256), 2, 20, CUS), "cd_life_kernel<7,sgn>"));
    // coupled constraints
    StreamShape coupled = bls(64);
    coupled.sep = false; coupled.queue_ok = false;
    p = stream_plan(coupled, defaults(), 2, 20, CUS);
    CHECK(!p.supported && !p.range_only);
    // the factor's rank: 288 columns at most, n >= 128
    CHECK(cd_life2_factor_ok(64, 288) && !cd_life2_factor_ok(64, 304) && !cd_life2_factor_ok(64, 289) && !cd_life2_factor_ok(7, 16) && !cd_life2_factor_ok(64, 0));
    CHECK(named(stream_plan(bls(1024), factor(304), 20, 4096, CUS), "cd_life_kernel<3,band>"));
    // the preloaded restarts: none on request, the budget's whole tiles at most
    w = factor(256); w.y0_max = 0;
    p = stream_plan(bls(1024), w, 20, 4096, CUS);
    CHECK(p.pre && p.y0_count == 0 && p.l2_y0 == 0 && p.l2_preslack == 20 * 4096);
    w.y0_max = 100;
    p = stream_plan(bls(1024), w, 20, 4096, CUS);
    CHECK(p.y0_count == 100 && p.l2_y0 == (size_t)7 * 16 * 256);
    w.y0_max = -5;
    CHECK(stream_plan(bls(1024), w, 20, 4096, CUS).y0_count == 0);
    const int64_t tiles288 = ((int64_t)2 << 30) / (18 * 16 * 16 * 8);
    p = stream_plan(bls(1024), factor(288), 256, 4096, CUS);          // 2^20 restarts at rank 288: 2.4 GB of Y0
    CHECK(p.pre && 256 * 4096 > 16 * tiles288 && p.y0_count == 16 * tiles288 && p.l2_y0 * 8 <= ((size_t)2 << 30) && p.l2_preslack == 256 * 4096);
    // the switches of the pre-pass, the tiles, the rotation, the tick sums
    w = factor(256); w.prebuilt = false;
    p = stream_plan(bls(1024), w, 20, 4096, CUS);
    CHECK(named(p, "cd_life_kernel<3,band,factored>") && !p.pre && p.y0_count == 0 && p.l2_preslack == 0);
    w = factor(256); w.tiles = 2; w.rot = 0; w.profile = true;
    p = stream_plan(bls(1024), w, 20, 4096, CUS);
    CHECK(named(p, "cd_life_kernel<3,band,2 tiles,factored>") && p.tiles == 2 && p.wgs == CUS && p.rot == 0 && p.life_prof == 24 && p.l2_scratch == (size_t)2 * CUS * 1024 * 16);
    w = defaults(); w.tiles = 2;
    CHECK(stream_plan(bls(1024), w, 20, 4096, CUS).tiles == 1);
    // debug switches: the generic kernels refuse the stream; the chain share's knob; the round-4 kernel's range
    w = defaults(); w.force_generic = true;
    CHECK(!stream_plan(bls(1024), w, 20, 4096, CUS).supported);
    w = defaults(); w.dbg = 64;
    CHECK(!stream_plan(bls(1024), w, 20, 4096, CUS).supported);
    w = defaults(); w.dbg = 128 | (2 << 8);
    CHECK(stream_plan(bls(512), w, 20, 4096, CUS).cs == 2);
    w.dbg = 128 | (6 << 8);
    CHECK(stream_plan(bls(512), w, 20, 4096, CUS).cs == 4);      // (cd_life_kernel is instantiated for 0, 2, 4)
    w.life_version = 1;
    CHECK(stream_plan(bls(512), w, 20, 4096, CUS).cs == 6);
    w.dbg = 128;
    p = stream_plan(bls(1024), w, 20, 4096, CUS);                 // 64 blocks on three SIMDs of 20
    CHECK(!p.supported && p.range_only);
    CHECK(chain_share(64, 0) == 4 && chain_share(64, 128 | (7 << 8)) == 6 && chain_share(64, 128 | (3 << 8)) == 2 && chain_share(3, 0) == 0 && chain_share(4, 0) == 0 && chain_share(5, 0) == 4);
    CHECK(chain_range_ok(64, 4) && !chain_range_ok(65, 4) && !chain_range_ok(64, 2) && !chain_range_ok(2, 0) && chain_range_ok(3, 0));
}

static void invariants(const StreamShape &s, const StreamSwitches &w, int64_t K, int64_t R) {
    const StreamPlan p = stream_plan(s, w, K, R, CUS);
    g_checked++;
    if (!p.supported) {
        CHECK(p.kernel == STREAM_NONE && p.l2_scratch == 0 && p.l2_preslack == 0 && p.l2_y0 == 0 && p.life_prof == 0 && p.outputs == 0 && p.bestK == 0);
        CHECK(!p.pre && !p.lr && p.y0_count == 0 && p.wgs == 0 && p.name[0] == 0);
        return;
    }
    CHECK(p.name[0] != 0 && p.outputs == (size_t)(K * R) && p.bestK == (size_t)K && p.wgs >= 1 && p.wgs <= (K * R + 15) / 16);
    CHECK(p.y0_count >= 0 && p.y0_count <= K * R && (p.y0_count % 16 == 0 || p.y0_count == K * R || p.y0_count == w.y0_max));
    if (p.kernel == STREAM_ROUND4) {
        CHECK(w.life_version == 1 && s.queue_ok && (p.cs == 0 || p.cs == 2 || p.cs == 4 || p.cs == 6) && (p.cs == 0 || p.cs < s.NB) && chain_range_ok(s.NB, p.cs));
        CHECK(!p.lr && !p.pre && p.l2_scratch == 0 && p.wgs <= CUS);
        return;
    }
    CHECK(p.kernel == STREAM_LIFE2 && w.life_version != 1 && !w.force_generic && !(w.dbg & 64));
    CHECK((p.nmw == 3 && (p.cs == 0 || p.cs == 2 || p.cs == 4)) || (p.nmw == 7 && p.cs == 4));
    CHECK(p.cs < s.NB && ((w.dbg & 128) || s.NB - p.cs <= (p.lr ? 256 : p.nmw * RQ_MAXU)));      // (the debug knob of the share is taken as it comes)
    if (p.lr) CHECK(p.nmw == 3 && p.cs == 0 && p.factor_rb == w.lr_RB && p.factor_rb <= L2_YBMAX && w.life_version != 3 && (p.kind == L2_KIND_BAND || p.kind == L2_KIND_GEN));
    CHECK(p.tiles == 1 || (p.tiles == 2 && p.lr));
    CHECK(p.wgs <= cd_life2_max_wgs(p.nmw, CUS, p.tiles));
    CHECK(p.l2_scratch >= (size_t)p.wgs * p.tiles * s.NB * 256);
    CHECK(!p.pre || p.lr);
    CHECK(p.pre ? (p.l2_preslack == (size_t)(K * R) && p.l2_y0 == (size_t)((p.y0_count + 15) / 16) * p.factor_rb * 256) : (p.l2_preslack == 0 && p.l2_y0 == 0 && p.y0_count == 0));
    CHECK(p.l2_y0 * sizeof(double) <= (size_t)L2_Y0_BUDGET);
}

int main() {
    table();
    const int dbgs[5] = {0, 64, 128, 128 | (2 << 8), 128 | (7 << 8) | 1024 | (5 << 12)};
    const int ranks[4] = {0, 1, 16, 19};
    const int classes[3] = {1, 4, 5};
    const long long y0s[3] = {STREAM_Y0_ALL, 100, 0};
    const int rots[4] = {STREAM_ROT_AUTO, 0, 1, 2};
    unsigned turn = 0;
    for (int NB = 1; NB <= 260; NB++)
        for (int maxc = 0; maxc <= 3; maxc++)
            for (int kc = 0; kc < 3; kc++)
                for (int objclass = 0; objclass <= 2; objclass++)
                    for (int bits = 0; bits < 4; bits++) {
                        StreamShape s;
                        s.NB = NB; s.sep = true; s.maxc = maxc; s.Kreal = classes[kc]; s.objclass = objclass; s.symcls = bits & 1; s.queue_ok = (bits & 2) != 0;
                        for (int lv = 0; lv <= 3; lv++)
                            for (int fg = 0; fg < 2; fg++)
                                for (int d = 0; d < 5; d++)
                                    for (int rk = 0; rk < 4; rk++)
                                        for (int pb = 0; pb < 2; pb++) {
                                            StreamSwitches w;
                                            w.life_version = lv; w.force_generic = fg != 0; w.dbg = dbgs[d]; w.lr_RB = ranks[rk]; w.prebuilt = pb != 0;
                                            // (what touches one field of the plan each takes turns)
                                            turn++;
                                            w.profile = turn & 1; w.y0_max = y0s[turn % 3]; w.rot = rots[(turn >> 1) & 3]; w.tiles = (turn & 4) ? 2 : 0;
                                            if (turn & 8) invariants(s, w, 2, 20); else invariants(s, w, 20, 4096);
                                        }
                    }
    StreamShape s = bls(64);
    s.sep = false;
    invariants(s, defaults(), 2, 20);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("ok %lld\n", g_checked);
    return 0;
}
