// Stand-alone check of qcqp_amd/csrc/batch_call.h on the CPU: built with the host compiler and the sanitizers, linked against the
// stand-in runtime below instead of libamdhip64.  The stand-ins back device memory with host memory (exact sizes: AddressSanitizer sees
// an overrun of the layout), log every call and can refuse the next allocation.  The structs below stand in for the kernels' argument
// structs (the record table goes by member names) and a host function for the kernel.  Exit status 0 and "ok" on stdout: every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../qcqp_amd/csrc/batch_call.h"

using namespace qcqpmi;

namespace {
struct Call { char kind; const void *dst, *src; size_t bytes; };      // 'u' upload, 'd' download, 'z' memset
std::vector<Call> calls;
std::set<void *> live;
int fail_next = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **ptr, size_t size) {
    if (fail_next > 0) { fail_next--; *ptr = nullptr; return hipErrorOutOfMemory; }
    *ptr = malloc(size);
    memset(*ptr, 0xA5, size);
    live.insert(*ptr);
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    if (p && !live.erase(p)) { fprintf(stderr, "free of a block that is not live\n"); abort(); }
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **, size_t, unsigned int) { abort(); }      // DevBuf<char> is not pinned
hipError_t hipHostFree(void *) { abort(); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    CHECK(kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToHost);
    calls.push_back({kind == hipMemcpyHostToDevice ? 'u' : 'd', dst, src, bytes});
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) {
    calls.push_back({'z', dst, nullptr, bytes});
    memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
}

namespace {

// the pointers of CdSmallArgs, AdmmSmallArgs and ChainStage that the record table names
struct CdK { int64_t *sweeps1, *sweeps2, *visits2, *accepted2; uint8_t *ran2; int *status1, *status2; double *f0, *maxviol; };
struct AdmmK { int64_t *iters1, *iters2; double *f0, *maxviol; };
struct StageK { int64_t *sweeps1, *sweeps2, *visits2, *accepted2; uint8_t *ran2; int *status1, *status2; int64_t *iters1, *iters2; double *f0, *maxviol; };

// ---- layout: the CD call of the worked example (B = 2, n = 5, R = 3, generated starts, shared constraints, best outputs wanted)
void check_layout() {
    const size_t B = 2, n = 5, R = 3, T = B * R;
    std::vector<double> P0s(B * n * n, 1.0), q0s(B * n, 2.0), r0s(B, 3.0), X(T * n, -1.0);
    const double *dP = (const double *)8, *dq = dP, *dr = dP, *dX0 = dP, *dcons = dP;
    double *dX = nullptr, *dkey = nullptr, *dbx = nullptr;
    int64_t *didx = nullptr;
    char *records = nullptr;
    int *ticket = nullptr;
    BatchCall f;
    const int iP = f.in(P0s.data(), B * n * n * 8, &dP), iq = f.in(q0s.data(), B * n * 8, &dq), ir = f.in(r0s.data(), B * 8, &dr);
    const int iX0 = f.in(nullptr, T * n * 8, &dX0);                     // generated starts: a missing input
    const int iX = f.out(X.data(), T * n * 8, &dX);
    const int irec = f.room(record_block_bytes<REC_CD>(T), &records);
    f.ticket(&ticket);
    const int iidx = f.room(B * 2 * 8, &didx), ikey = f.room(B * 2 * 8, &dkey), ibx = f.room(B * n * 8, &dbx);
    const int icons = f.in(nullptr, B * 7 * 24, &dcons);
    CHECK(record_block_bytes<REC_CD>(T) == T * 57);
    const size_t want[] = {512, 256, 256, 0, 256, 512, 256, 256, 256, 256, 0};
    const int order[] = {iP, iq, ir, iX0, iX, irec, f.iticket, iidx, ikey, ibx, icons};
    size_t off = 0;
    for (int k = 0; k < 11; k++) {
        CHECK(order[k] == k && f.pieces[(size_t)k].off == off && off % 256 == 0);      // declaration order, 256-aligned, an empty piece takes no room
        off += want[k];
    }
    // the pieces sum to 2816 (the old Carve, whose take() this is, asks for the same)
    size_t carve = 0;
    for (size_t bytes : {B * n * n * 8, B * n * 8, B * 8, (size_t)0, T * n * 8, T * 57, 2 * sizeof(int), B * 2 * 8, B * 2 * 8, B * n * 8, (size_t)0}) carve += (bytes + 255) / 256 * 256;
    CHECK(f.total == 2816 && off == 2816 && carve == 2816);
    // no pointer before the reserve -- and none after one that failed; nothing enqueued either
    CHECK(!dP && !dq && !dr && !dX0 && !dX && !records && !ticket && !didx && !dkey && !dbx && !dcons && !f.w);
    DevBuf<char> buf;
    fail_next = 1;
    CHECK(f.reserve(buf, nullptr) == hipErrorOutOfMemory);
    CHECK(!dP && !dX && !records && !ticket && !dbx && !f.w && calls.empty() && live.empty());
    CHECK(f.reserve(buf, nullptr) == hipSuccess && buf.cap == 2816 && f.w == buf.p && calls.empty());
    CHECK((const char *)dP == buf.p && (const char *)dq == buf.p + 512 && (char *)dX == buf.p + 1024 && records == buf.p + 1280 &&
          (char *)ticket == buf.p + 1792 && (char *)dbx == buf.p + 2560);
    CHECK(!dX0 && !dcons);                                              // an empty piece has no address
    // uploads in declaration order, missing ones skipped, then the ticket: ONE memset of 8 bytes
    CHECK(f.upload(nullptr) == hipSuccess && calls.size() == 4);
    CHECK(calls[0].kind == 'u' && calls[0].dst == dP && calls[0].src == P0s.data() && calls[0].bytes == 400);
    CHECK(calls[1].kind == 'u' && calls[1].dst == dq && calls[1].bytes == 80 && calls[2].kind == 'u' && calls[2].dst == dr && calls[2].bytes == 16);
    CHECK(calls[3].kind == 'z' && calls[3].dst == ticket && calls[3].bytes == 8 && ticket[0] == 0 && ticket[1] == 0);
    CHECK(dP[0] == 1.0 && dq[9] == 2.0 && dr[1] == 3.0);
    // downloads: the one output with a destination
    for (size_t i = 0; i < T * n; i++) dX[i] = (double)i;
    calls.clear();
    CHECK(f.download(nullptr) == hipSuccess && calls.size() == 1 && calls[0].kind == 'd' && calls[0].dst == X.data() && calls[0].src == dX && calls[0].bytes == 240);
    CHECK(X[0] == 0.0 && X[T * n - 1] == (double)(T * n - 1));
    calls.clear();
    // an input with a source but no bytes, an output without a destination or without bytes, a fetch out of layout order
    BatchCall g;
    const double *e0 = nullptr;
    double *o0 = nullptr, *o1 = nullptr, *o2 = nullptr, *o3 = nullptr;
    double host1[4] = {0, 0, 0, 0}, host3[2] = {0, 0};
    g.in(P0s.data(), 0, &e0);
    g.out(nullptr, 32, &o0);
    const int late = g.room(32, &o1);
    g.out(host1, 0, &o2);
    g.out(host3, 16, &o3);
    g.fetch(late, host1);
    DevBuf<char> buf2;
    CHECK(g.total == 768 && g.reserve(buf2, nullptr) == hipSuccess && !e0 && o0 && o1 == o0 + 32 && !o2 && o3 == o0 + 64 && g.iticket < 0);
    CHECK(g.upload(nullptr) == hipSuccess && calls.empty());            // nothing to upload, no ticket declared
    o1[3] = 7.0; o3[1] = 9.0;
    CHECK(g.download(nullptr) == hipSuccess && calls.size() == 2 && calls[0].dst == host3 && calls[0].bytes == 16 && calls[1].dst == host1 && calls[1].bytes == 32);
    CHECK(host1[3] == 7.0 && host3[1] == 9.0);
    calls.clear();
}

// ---- records: a recognisable value per (array, stage, restart)
template <class T> T code(int field, size_t stage, size_t r) { return (T)(field * 10000 + (int)stage * 100 + (int)r + 1); }
template <> uint8_t code<uint8_t>(int, size_t stage, size_t r) { return (uint8_t)(stage * 16 + r + 1); }

// every array of a block, host side: exactly `count` entries each (AddressSanitizer sees an unpack that runs over), or absent
struct HostArrays {
    std::vector<int64_t> i64[6];
    std::vector<double> f64[2];
    std::vector<int> i32[2];
    std::vector<uint8_t> u8;
    RecordsOut out(size_t count, unsigned absent) {      // bit k of absent: array k of RecordsOut is not wanted
        for (auto &v : i64) v.assign(count, -1);
        for (auto &v : f64) v.assign(count, -1.0);
        for (auto &v : i32) v.assign(count, -1);
        u8.assign(count, 255);
        auto w = [absent](unsigned k, auto &v) { return absent >> k & 1 ? nullptr : v.data(); };
        return {w(0, i64[0]), w(1, i64[1]), w(2, i64[2]), w(3, i64[3]), w(4, i64[4]), w(5, i64[5]), w(6, f64[0]), w(7, f64[1]), w(8, i32[0]), w(9, i32[1]), w(10, u8)};
    }
};

template <class T> void expect(const std::vector<T> &v, bool written, int field, size_t stages, size_t T_) {
    for (size_t s = 0; s < stages; s++)
        for (size_t r = 0; r < T_; r++) CHECK(v[s * T_ + r] == (written ? code<T>(field, s, r) : (T)-1));
}

// the stand-in kernel: stage s, restart r, through the pointers the frame handed out
template <class K> void write_cd(K &k, size_t s, size_t r) {
    k.sweeps1[r] = code<int64_t>(0, s, r); k.sweeps2[r] = code<int64_t>(1, s, r); k.visits2[r] = code<int64_t>(2, s, r); k.accepted2[r] = code<int64_t>(3, s, r);
    k.status1[r] = code<int>(8, s, r); k.status2[r] = code<int>(9, s, r); k.ran2[r] = code<uint8_t>(10, s, r);
}
template <class K> void write_admm(K &k, size_t s, size_t r) { k.iters1[r] = code<int64_t>(4, s, r); k.iters2[r] = code<int64_t>(5, s, r); }
template <class K> void write_values(K &k, size_t s, size_t r) { k.f0[r] = code<double>(6, s, r); k.maxviol[r] = code<double>(7, s, r); }

// one block of WHICH with `stages` stages of T restarts behind an odd-sized piece; `absent`: destinations left null
template <int WHICH, class K>
void round_trip(size_t T_, size_t stages, unsigned absent) {
    const size_t count = stages * T_, bytes = record_block_bytes<WHICH>(count);
    CHECK(bytes == count * (WHICH == REC_CD ? 57 : WHICH == REC_ADMM ? 32 : 73));
    BatchCall f;
    char *pad = nullptr, *records = nullptr;
    int *ticket = nullptr;
    f.room(3, &pad);
    f.room(bytes, &records);
    f.ticket(&ticket);
    DevBuf<char> buf;
    CHECK(f.reserve(buf, nullptr) == hipSuccess && f.upload(nullptr) == hipSuccess);
    memset(records, 0, bytes);
    std::vector<K> k(stages);
    for (size_t s = 0; s < stages; s++) {
        bind_records<WHICH>(k[s], records, T_, stages, s);
        for (size_t r = 0; r < T_; r++) {
            if constexpr ((WHICH & REC_CD) != 0) write_cd(k[s], s, r);
            if constexpr ((WHICH & REC_ADMM) != 0) write_admm(k[s], s, r);
            write_values(k[s], s, r);
        }
    }
    CHECK(ticket[0] == 0 && ticket[1] == 0 && pad[0] == (char)0xA5);    // the kernel wrote inside its block
    std::vector<char> hout(bytes);
    CHECK(hipMemcpyAsync(hout.data(), records, bytes, hipMemcpyDeviceToHost, nullptr) == hipSuccess);
    HostArrays h;
    const RecordsOut out = h.out(count, absent);
    unpack_records<WHICH>(out, hout.data(), count, 0, count);
    const bool cd = (WHICH & REC_CD) != 0, admm = (WHICH & REC_ADMM) != 0;
    for (int k4 = 0; k4 < 4; k4++) expect(h.i64[k4], cd && !(absent >> k4 & 1), k4, stages, T_);
    for (int k2 = 4; k2 < 6; k2++) expect(h.i64[k2], admm && !(absent >> k2 & 1), k2, stages, T_);
    for (int k2 = 6; k2 < 8; k2++) expect(h.f64[k2 - 6], !(absent >> k2 & 1), k2, stages, T_);
    for (int k2 = 8; k2 < 10; k2++) expect(h.i32[k2 - 8], cd && !(absent >> k2 & 1), k2, stages, T_);
    for (size_t s = 0; s < stages; s++)
        for (size_t r = 0; r < T_; r++) CHECK(h.u8[s * T_ + r] == (cd && !(absent >> 10 & 1) ? code<uint8_t>(10, s, r) : 255));
    // the last stage's rows of f0 / maxviol, as the chain hands out its final values
    std::vector<double> f0(T_, -1.0), maxviol(T_, -1.0);
    RecordsOut rows = {};
    rows.f0 = f0.data();
    if (!(absent >> 7 & 1)) rows.maxviol = maxviol.data();
    unpack_records<WHICH>(rows, hout.data(), count, (stages - 1) * T_, T_);
    for (size_t r = 0; r < T_; r++) CHECK(f0[r] == code<double>(6, stages - 1, r) && maxviol[r] == (absent >> 7 & 1 ? -1.0 : code<double>(7, stages - 1, r)));
    calls.clear();
}

void check_records() {
    for (size_t T_ : {1, 3, 5})
        for (unsigned absent : {0u, 0x555u, 0x2aau, 0x7ffu}) {
            round_trip<REC_CD, CdK>(T_, 1, absent);
            round_trip<REC_ADMM, AdmmK>(T_, 1, absent);
            round_trip<REC_CD | REC_ADMM, StageK>(T_, 1, absent);
            round_trip<REC_CD | REC_ADMM, StageK>(T_, 3, absent);
        }
}

// ---- ticket_partition against the arithmetic of the drivers before the header existed
void reference_partition(int64_t B, int64_t R, int wgs, int64_t waves, int64_t *RC, int64_t *chunks, int *out_wgs) {
    int64_t ch = B >= wgs ? 1 : (wgs + B - 1) / B;
    if (ch > (R + waves - 1) / waves) ch = (R + waves - 1) / waves;
    *RC = (R + ch - 1) / ch;
    *chunks = (R + *RC - 1) / *RC;
    *out_wgs = wgs > B * *chunks ? (int)(B * *chunks) : wgs;
}

void check_tickets() {
    for (int64_t B = 1; B <= 40; B++)
        for (int64_t R = 1; R <= 70; R++)
            for (int wgs : {1, 3, 256, 1024})
                for (int64_t waves : {4, 8}) {
                    const TicketPlan t = ticket_partition(B, R, wgs, waves);
                    int64_t RC, chunks;
                    int w;
                    reference_partition(B, R, wgs, waves, &RC, &chunks, &w);
                    CHECK(t.RC == RC && t.chunks == chunks && t.wgs == w);
                    CHECK(t.chunks * t.RC >= R && (t.chunks - 1) * t.RC < R && 1 <= t.wgs && t.wgs <= B * t.chunks);
                }
}

// ---- 256 threads or the large workgroup: more waves per CU wins, a tie goes to the larger
void check_wide_threads() {
    const int table[][3] = {{3, 1, 256}, {4, 1, 256}, {1, 0, 256}, {5, 2, 256}, {2, 1, 512}, {1, 1, 512}, {0, 0, 512}, {4, 2, 512}, {3, 2, 512}, {0, 1, 512}};
    for (const auto &row : table) CHECK(batch_wide_threads(row[0], row[1], 512) == row[2]);
    CHECK(batch_wide_threads(3, 1, 768) == 768 && batch_wide_threads(4, 1, 768) == 256);
}

// ---- the names qcqpmi_last_cd_kernel and qcqpmi_admm_last_kernel hand out: the literal strings, from storage that stays
void check_names() {
    const char *cd[8] = {"cd_small_kernel<1>", "cd_small_kernel<1,w2>", "cd_small_kernel<1,pc>", "cd_small_kernel<1,pc,w2>",
                         "cd_small_kernel<4>", "cd_small_kernel<4,w2>", "cd_small_kernel<4,pc>", "cd_small_kernel<4,pc,w2>"};
    const char *admm[8] = {"admm_small_kernel<1>", "admm_small_kernel<1,w2>", "admm_small_kernel<1,pc>", "admm_small_kernel<1,pc,w2>",
                           "admm_small_kernel<4>", "admm_small_kernel<4,w2>", "admm_small_kernel<4,pc>", "admm_small_kernel<4,pc,w2>"};
    const char *chain[4] = {"chain_small_kernel<1>", "chain_small_kernel<1,pc>", "chain_small_kernel<4>", "chain_small_kernel<4,pc>"};
    for (int v = 0; v < 8; v++) {
        const int maxc = v & 4 ? 3 : 1;      // the drivers pass 1 or 4; anything above 1 is the <4> kernel
        const char *a = batch_kernel_name<CdK>("cd_small_kernel", maxc, (v & 2) != 0, (v & 1) != 0);
        CHECK(std::string(a) == cd[v] && a == batch_kernel_name<CdK>("cd_small_kernel", maxc, (v & 2) != 0, (v & 1) != 0));
        CHECK(std::string(batch_kernel_name<AdmmK>("admm_small_kernel", v & 4 ? 4 : 0, (v & 2) != 0, (v & 1) != 0)) == admm[v]);
        if (!(v & 1)) CHECK(std::string(batch_kernel_name<StageK>("chain_small_kernel", v & 4 ? 4 : 1, (v & 2) != 0, false)) == chain[v >> 1]);
    }
}

}  // namespace

int main() {
    check_layout();
    check_records();
    check_tickets();
    check_wide_threads();
    check_names();
    CHECK(live.empty() && calls.empty());
    printf("ok\n");
    return 0;
}
