// The decision of a streamed coordinate-descent run (qcqpmi_cd_stream_run / qcqpmi_cd_stream_reserve, capi_stream.hip): which kernel,
// which instantiation, which pre-passes, how many workgroups, which buffers of what size -- as plain C++ on a handful of integers (no HIP
// include, like p1_bisect.h), so that a host program can drive it: tests/host/stream_plan_selftest.cpp.  Reserve and run both ask
// stream_plan and nothing else; the constants and the step kinds the rules read have their one definition here (cd_roles.h, cd_life.h
// and cd_life.hip include this header).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qcqpmi {

constexpr int RQ_NSIMD = 3;   // SIMDs that multiply (the fourth runs the chain)
constexpr int RQ_MAXU = 20;   // blocks one SIMD can own (<= RQ_RND * RQ_PFU): n = 1024 needs the chain to take >= 4 blocks.
                              // (22 units = 5 passes + 2 re-read units measured 2.5 % slower at the same split, and smaller
                              //  chain shares do not pay: the mfma waves become the bottleneck)
constexpr int RQ_CSMAX = 6;   // blocks the chain wave can own
constexpr int L2_YBMAX = 18;  // blocks of 16 rows of Y a tile can hold: factor rank <= 288
constexpr int L2_KCL = 4;     // constraint classes of the multi-class kinds (GENK / LINK); up to two constraints per coordinate

// step kinds.  GENK / LINK (round 6): GEN / LIN for problems with SEVERAL constraint classes (coordinates with different
// constraint lists: up to four classes) and up to two constraints per coordinate -- the slots keep a feasible set per class, the
// chain looks its columns' classes up per block
// SGN: a diagonal of P0 of MIXED sign (a box-constrained QP with an indefinite P0), one class with one constraint per coordinate:
// the step is the GEN pick where P0[i,i] > 0, the outermost end point on the far side of the vertex where P0[i,i] < 0 (a concave scalar
// objective), the LIN pick where P0[i,i] == 0; the objective is tracked as an absolute value like LIN's (a frozen sweep first)
enum { L2_KIND_BAND = 0, L2_KIND_GEN = 1, L2_KIND_LIN = 2, L2_KIND_GENK = 3, L2_KIND_LINK = 4, L2_KIND_SGN = 5 };

// ---- the role-split phase-2 kernels (cd_phase2_q_kernel, cd_phase2_qs_kernel): the chain wave's share of the contraction
// blocks of the contraction the chain wave multiplies, of NB: four, or the debug knob's (dbg & 128: bits 8-10), at most RQ_CSMAX, none
// when the share would be the whole contraction, even
inline int chain_share(int NB, int dbg) {
    int cs = (dbg & 128) ? ((dbg >> 8) & 7) : 4;     // debug knob: blocks of the contraction the chain wave multiplies
    cs = cs > RQ_CSMAX ? RQ_CSMAX : cs;
    if (cs >= NB) cs = 0;
    cs &= ~1;
    return cs;
}

// do the three multiplying SIMDs hold the blocks the chain leaves them?  (n <= 1024 with a share of four; at least 3 blocks of 16)
inline bool chain_range_ok(int NB, int cs) { return NB - cs <= RQ_NSIMD * RQ_MAXU && NB >= 3; }

// ---- cd_life_kernel (cd_life.h): the shape rules
// can the factored-objective kernel take a factor of r columns for a problem of NB blocks?  (rank, the scratch of the column build)
inline bool cd_life2_factor_ok(int NB, int64_t r) {
    const int64_t r16 = (r + 15) / 16 * 16;
    if (r < 1 || r16 > 16 * L2_YBMAX || NB < 8) return false;
    return true;
}

inline int cd_life2_max_wgs(int nmw, int cus, int tiles) { return (nmw == 3 && tiles == 1) ? 2 * cus : cus; }

// does the kernel take this problem?  nmw / cs / kind: the instantiation (multiplying waves 3 | 7, chain share, step kind)
// sep, maxc: separable constraints, the most on one coordinate; Kreal: constraint classes among the real coordinates
// objclass: 1 = P0[i,i] > 0 everywhere, 2 = zero everywhere, 0 = anything else (mixed signs: the SGN kind, one class with one
// constraint per coordinate only, never with a factor)
// factor_rb: blocks of 16 rows of an objective factor the caller WILL hand over (0: none) -- the factored instantiation keeps Y, not X,
// in registers, so with a factor the kernel also takes 2304 < n <= 4096 (and prefers three multiplying waves from n = 1040 on)
inline bool cd_life2_config(int NB, bool sep, int maxc, int Kreal, int objclass, bool symcls, int factor_rb, int *nmw, int *cs, int *kind) {
    // one class with one constraint per coordinate: the BAND / GEN / LIN kinds; up to L2_KCL classes with up to two constraints per
    // coordinate (every real coordinate constrained): GENK / LINK
    if (!sep || maxc < 1 || maxc > 2 || Kreal < 1 || Kreal > L2_KCL) return false;
    const bool multi = maxc > 1 || Kreal > 1;
    // objclass 0 = a diagonal of mixed sign (or zero in places): the SGN kind, one class with one constraint per coordinate only
    if (objclass != 0 && objclass != 1 && objclass != 2) return false;
    if (objclass == 0 && multi) return false;
    if (NB < 3) return false;
    int w, c;
    if (NB <= 4) { w = 3; c = 0; }
    else if (NB - 4 <= 3 * RQ_MAXU) { w = 3; c = (NB < 8) ? 2 : 4; }
    else if (factor_rb > 0 && !multi && objclass == 1 && NB <= 256) { w = 3; c = 0; }      // factored: nothing in its registers grows with n
    else if (NB - 4 <= 7 * RQ_MAXU) { w = 7; c = 4; }
    else return false;
    *nmw = w; *cs = c;
    *kind = objclass == 0 ? L2_KIND_SGN : multi ? (objclass == 2 ? L2_KIND_LINK : L2_KIND_GENK) : objclass == 2 ? L2_KIND_LIN : (symcls ? L2_KIND_BAND : L2_KIND_GEN);
    return true;
}

// tiles of 16 slots per workgroup (1 | 2); requested: 0 = automatic (QCQPMI_L2_TILES: experiments).  Two tiles per workgroup -- one
// eight-wave workgroup per CU, joint episodes, the build by 512 threads -- exist for the factored objective only and are NOT the default:
// measured at n = 1024 (20 x 4096 restarts) 33.7-35.4 ms against 32.6-34.4 ms for two four-wave workgroups per CU, whose column builds
// overlap the neighbour's products (profiles/r06_summary.md; without a factor: 52.0-53.5 against 49.5-51.0 ms,
// profiles/r06_headline_experiments.md -- that instantiation was removed).
inline int cd_life2_tiles(int nmw, int cs, int requested, int lr) {
    if (!lr || nmw != 3 || cs != 0) return 1;
    return requested == 2 ? 2 : 1;
}

inline const char *cd_life2_name(int nmw, int kind, int tiles, int lr) {
    if (kind == L2_KIND_GENK) return nmw == 3 ? "cd_life_kernel<3,gen,classes>" : "cd_life_kernel<7,gen,classes>";
    if (kind == L2_KIND_LINK) return nmw == 3 ? "cd_life_kernel<3,lin,classes>" : "cd_life_kernel<7,lin,classes>";
    if (kind == L2_KIND_SGN) return nmw == 3 ? "cd_life_kernel<3,sgn>" : "cd_life_kernel<7,sgn>";
    if (lr) return tiles == 2 ? (kind == L2_KIND_BAND ? "cd_life_kernel<3,band,2 tiles,factored>" : "cd_life_kernel<3,gen,2 tiles,factored>")
                              : (kind == L2_KIND_BAND ? "cd_life_kernel<3,band,factored>" : "cd_life_kernel<3,gen,factored>");
    if (tiles == 2) return kind == L2_KIND_BAND ? "cd_life_kernel<3,band,2 tiles>" : kind == L2_KIND_GEN ? "cd_life_kernel<3,gen,2 tiles>" : "cd_life_kernel<3,lin,2 tiles>";
    if (nmw == 3) return kind == L2_KIND_BAND ? "cd_life_kernel<3,band>" : kind == L2_KIND_GEN ? "cd_life_kernel<3,gen>" : "cd_life_kernel<3,lin>";
    return kind == L2_KIND_BAND ? "cd_life_kernel<7,band>" : kind == L2_KIND_GEN ? "cd_life_kernel<7,gen>" : "cd_life_kernel<7,lin>";
}

// Preloaded restarts of a prebuilt factored run of KR restarts (CdLife::y0_count): the leading ones, as many as y0_max allows
// (QCQPMI_L2_Y0_MAX; unset = STREAM_Y0_ALL: all; 0: none -- every restart takes its loading sweep inside the launch, the A / B reference)
// and as fit L2_Y0_BUDGET bytes of Y0 (whole tiles of 16 restarts x 16 RB rows; the headline's 81 920 restarts at rank 256 take 168 MB).
// The rest load in-kernel: the same bits either way, no second code path.
constexpr int64_t L2_Y0_BUDGET = (int64_t)2 << 30;
constexpr long long STREAM_Y0_ALL = 0x7fffffffffffffffLL;
inline int64_t cd_life2_y0_count(int64_t KR, int RB, long long y0_max) {
    int64_t cnt = KR;
    { const long long m = y0_max; cnt = m < 0 ? 0 : (m < cnt ? m : cnt); }
    const int64_t fit = L2_Y0_BUDGET / ((int64_t)RB * 16 * 16 * (int64_t)sizeof(double)) * 16;
    return cnt < fit ? cnt : fit;
}

// ---- the plan
struct StreamShape {             // what the decision reads of the problem
    int NB;                      // blocks of 16 coordinates (n16 / 16)
    bool sep;                    // every constraint touches one coordinate
    int maxc, Kreal, objclass;   // constraints on one coordinate at most; classes among the real coordinates; the diagonal of P0 (cd_life2_config)
    bool symcls;                 // one class of the form p x_i^2 + r == 0
    bool queue_ok;               // the round-4 kernel takes the shape (cd_queue_shape_ok: the rule of qcqpmi_cd_run's queue kernel)
};

constexpr int STREAM_ROT_AUTO = -0x7fffffff - 1;
struct StreamSwitches {          // ... and besides the problem: the context's switches and the environment, parsed (stream_switches)
    int life_version;            // qcqpmi_cd_life_version
    bool force_generic;          // qcqpmi_debug_profile
    int dbg;
    int lr_RB;                   // blocks of 16 columns of the objective factor that is set (0: none)
    bool profile;
    bool prebuilt;               // QCQPMI_L2_PREBUILT (unset: on)
    long long y0_max;            // QCQPMI_L2_Y0_MAX (unset: STREAM_Y0_ALL)
    int rot;                     // QCQPMI_L2_ROT (unset: STREAM_ROT_AUTO)
    int tiles;                   // QCQPMI_L2_TILES (unset: 0, automatic)
};

enum { STREAM_NONE = 0, STREAM_LIFE2 = 1, STREAM_ROUND4 = 2 };      // cd_life_kernel | cd_phase2_qs_kernel<CS, lifecycle>

struct StreamPlan {
    bool supported;
    bool range_only;             // refused for nothing but n outside the round-4 kernel's range (a message of its own)
    int kernel;                  // STREAM_*
    int nmw, cs, kind;           // cd_life_kernel's instantiation; cs: also the round-4 kernel's
    bool lr;                     // the factored instantiation
    int factor_rb;               // blocks of 16 rows of the factor the run uses (0: none)
    bool pre;                    // the column build and Y0 ahead of the launch (cd_life_prep_kernel, cd_life_y0_kernel)
    int tiles;
    int64_t wgs;
    int64_t y0_count;
    int rot;                     // what the second workgroup of a CU does with its roles (cd_life.h: CdLife2Args::rotmode)
    const char *name;
    // elements of the buffers the run reserves (0: not needed)
    size_t l2_scratch, l2_preslack, l2_y0, life_prof;
    size_t outputs;              // restarts whose outputs are staged
    size_t bestK;                // populations whose winners are kept
};

// the decision for K populations of R restarts on a device of `cus` compute units
inline StreamPlan stream_plan(const StreamShape &sh, const StreamSwitches &sw, int64_t K, int64_t R, int cus) {
    StreamPlan p = StreamPlan();
    p.name = "";
    const int NB = sh.NB;
    int nmw = 0, cs2 = 0, kind = 0;
    const int factor_rb = (sw.lr_RB > 0 && sw.life_version != 3 && cd_life2_factor_ok(NB, 16 * (int64_t)sw.lr_RB)) ? sw.lr_RB : 0;
    const bool use2 = sw.life_version != 1 && !sw.force_generic && !(sw.dbg & 64) && sh.sep &&
                      cd_life2_config(NB, sh.sep, sh.maxc, sh.Kreal, sh.objclass, sh.symcls, factor_rb, &nmw, &cs2, &kind);
    // ONE lifecycle kernel (round 6): cd_life_kernel takes every shape the round-4 kernel (cd_phase2_qs_kernel<CS, lifecycle>, cd_queue.hip)
    // takes and more; the shape rule of round 5 (the round-4 kernel from n = 960 on for runs beyond 8192 restarts, where it is 12 % faster
    // on a FULL-rank objective: profiles/r05_life_vs_round4.md) is gone -- the headline family has a low-rank objective and runs the
    // factored instantiation, 1.3 x faster than either (profiles/r06_summary.md).  qcqpmi_cd_life_version(1) still launches the round-4
    // kernel: a debug switch, kept as the independent implementation the tests compare against.
    if (!use2) {
        // (qcqpmi_cd_queue chooses the phase-2 kernel of qcqpmi_cd_run; it does not apply here)
        const bool eligible = !sw.force_generic && !(sw.dbg & 64) && sh.queue_ok && NB - 4 <= RQ_NSIMD * RQ_MAXU && NB >= 3;
        if (!eligible || sw.life_version != 1) return p;
        const int cs = chain_share(NB, sw.dbg);
        if (!chain_range_ok(NB, cs)) { p.range_only = true; return p; }
        p.supported = true; p.kernel = STREAM_ROUND4; p.cs = cs;
        p.wgs = (K * R + 15) / 16 < cus ? (K * R + 15) / 16 : cus;
        p.name = "cd_phase2_qs_kernel<lifecycle>";
    } else {
        // factored objective (qcqpmi_cd_set_objective_factor): cd_life_kernel's products through Y = L^T X -- half the matrix work and less
        // per block interval, a positive diagonal (band / gen kinds), three multiplying waves per tile
        const bool lr = factor_rb > 0 && nmw == 3 && (kind == L2_KIND_BAND || kind == L2_KIND_GEN);
        if (lr) cs2 = 0;
        // the debug knob of the chain share, by cd_life_kernel's own rule: the shares it is instantiated for, four-wave workgroups only
        if (!lr && (sw.dbg & 128)) { const int k2 = (sw.dbg >> 8) & 7; if (nmw == 3 && (k2 == 0 || k2 == 2 || k2 == 4) && k2 < NB) cs2 = k2; }
        p.supported = true; p.kernel = STREAM_LIFE2; p.nmw = nmw; p.cs = cs2; p.kind = kind; p.lr = lr; p.factor_rb = factor_rb;
        // the factored instantiation builds its columns ahead of the launch (cd_life_prep_kernel, every restart of the run at full
        // occupancy) and its refill only copies them; QCQPMI_L2_PREBUILT=0: the build inside the launch, as before (A / B runs, tests)
        p.pre = lr && sw.prebuilt;
        p.y0_count = p.pre ? cd_life2_y0_count(K * R, factor_rb, sw.y0_max) : 0;
        p.tiles = cd_life2_tiles(nmw, cs2, sw.tiles, lr ? 1 : 0);
        p.wgs = (K * R + 16 * p.tiles - 1) / (16 * p.tiles);
        const int maxw = cd_life2_max_wgs(nmw, cus, p.tiles);
        if (p.wgs > maxw) p.wgs = maxw;
        if (sw.dbg & 1024) { const int lim = (sw.dbg >> 12) & 1023; if (lim > 0 && p.wgs > lim) p.wgs = lim; }     // debug knob: workgroups of the launch
        // which of its CU's two workgroups a workgroup is (arrival counter per CU, HW_ID), and what the second one does with it:
        //   QCQPMI_L2_ROT=2 (the default with the factored objective): it turns its MULTIPLYING roles by one among SIMDs 1-3 -- 16 blocks of Y
        //   are 6 + 5 + 5 over the three waves, and with both six-block waves on SIMD 1 that SIMD's matrix pipe was 83 % busy and late for
        //   one product in ten: the chain's wait for partial tiles 0.76 k -> 0.57 k cycles per block interval, the interval 7.45 k -> 7.29 k
        //   (A / B / A / B on one box: 32.93 / 32.57 / 32.80 / 32.45 ms per 20 x 4096 restarts; same bits);
        //   QCQPMI_L2_ROT=1: it turns ALL roles by two SIMDs (the two chains on different SIMDs) -- measured SLOWER, 33.2 -> 35.7 ms: a chain
        //   beside a product stream waits behind the stream's queued matrix instructions (profiles/r06_summary.md);  0: off
        p.rot = sw.rot != STREAM_ROT_AUTO ? sw.rot : (lr ? 2 : 0);
        p.name = cd_life2_name(nmw, kind, p.tiles, lr ? 1 : 0);
        // the workgroups' X tiles (two tiles per workgroup: half the workgroups, the same tiles)
        p.l2_scratch = (size_t)cd_life2_max_wgs(nmw, cus, 1) * (size_t)NB * 256;
        if (p.pre) {
            p.l2_preslack = (size_t)(K * R);
            p.l2_y0 = (size_t)((p.y0_count + 15) / 16) * (size_t)factor_rb * 256;
        }
    }
    p.life_prof = sw.profile ? 24 : 0;
    p.outputs = (size_t)(K * R);
    p.bestK = (size_t)K;
    return p;
}

}  // namespace qcqpmi
