// RCCL part of the C ABI: the lazily loaded library, the communicator of a context and the qcqpmi_comm_* calls.  Host code
// only, and the one unit that includes rccl/rccl.h.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstring>

#include "capi_ctx.h"

using namespace qcqpmi;

namespace {

struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi *rccl() {
    static RcclApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char *nm : names) {
            api.h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
            if (api.h) break;
        }
        if (api.h) {
            api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.h, "ncclGetUniqueId");
            api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.h, "ncclCommInitRank");
            api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.h, "ncclCommDestroy");
            api.AllGather = (decltype(api.AllGather))dlsym(api.h, "ncclAllGather");
            api.Broadcast = (decltype(api.Broadcast))dlsym(api.h, "ncclBroadcast");
            api.AllReduce = (decltype(api.AllReduce))dlsym(api.h, "ncclAllReduce");
            api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.h, "ncclGetErrorString");
        }
    }
    return (api.h && api.GetUniqueId && api.CommInitRank && api.AllGather && api.Broadcast &&
            api.AllReduce) ? &api : nullptr;
}

}  // namespace

// qcqpmi_ctx_destroy: the communicator goes with the context
void qcqpmi::comm_drop(qcqpmi_ctx *c) {
    if (c->comm && rccl() && rccl()->CommDestroy) rccl()->CommDestroy(c->comm);
    c->comm = nullptr;
}

extern "C" {

#define NCCLCHK(c, expr)                                                                        \
    do {                                                                                        \
        ncclResult_t r_ = (expr);                                                               \
        if (r_ != ncclSuccess)                                                                  \
            return fail(c, QCQPMI_ECOMM, "%s failed: %s", #expr,                                \
                        rccl()->GetErrorString ? rccl()->GetErrorString(r_) : "rccl error");    \
    } while (0)

int qcqpmi_comm_unique_id(uint8_t id_out[128]) {
    if (!rccl()) return fail(nullptr, QCQPMI_ECOMM, "librccl.so could not be loaded");
    ncclUniqueId id;
    if (rccl()->GetUniqueId(&id) != ncclSuccess) return fail(nullptr, QCQPMI_ECOMM, "ncclGetUniqueId failed");
    memcpy(id_out, id.internal, 128);
    return 0;
}

int qcqpmi_comm_init(qcqpmi_ctx *c, int rank, int world, const uint8_t id_in[128]) {
    if (!c || world < 1 || rank < 0 || rank >= world) return QCQPMI_EINVAL;
    if (!rccl()) return fail(c, QCQPMI_ECOMM, "librccl.so could not be loaded");
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(id.internal, id_in, 128);
    NCCLCHK(c, rccl()->CommInitRank(&c->comm, world, id, rank));
    c->rank = rank; c->world = world;
    HIPCHK(c, c->d_comm.reserve(c->stream, (size_t)4 * world + 4 + (size_t)c->n));
    return 0;
}

int qcqpmi_comm_barrier(qcqpmi_ctx *c) {
    double v = 0.0;
    return qcqpmi_comm_allreduce(c, &v, 1, 0);
}

int qcqpmi_comm_allreduce(qcqpmi_ctx *c, double *values, int64_t count, int op) {
    if (!c || !values || count < 1 || count > ((int64_t)1 << 28) || op < 0 || op > 1) return QCQPMI_EINVAL;
    if (!c->comm) return fail(c, QCQPMI_ESTATE, "comm_init has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    double *buf = c->d_comm;
    if (count > 4) {      // the exchange of a streamed run (keys of all populations, then the winners' points): a buffer of its own
        HIPCHK(c, c->d_comm_big.reserve(c->stream, (size_t)count, false));
        buf = c->d_comm_big;
    }
    HIPCHK(c, hipMemcpyAsync(buf, values, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, rccl()->AllReduce(buf, buf, (size_t)count, ncclDouble, op == 0 ? ncclMax : ncclSum, c->comm, c->stream));
    HIPCHK(c, hipMemcpyAsync(values, buf, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

// every rank contributes `nbytes` bytes; everyone receives the world x nbytes bytes in rank order (one ncclAllGather)
int qcqpmi_comm_allgather(qcqpmi_ctx *c, const void *send, int64_t nbytes, void *recv) {
    if (!c || !send || !recv || nbytes < 1 || nbytes > ((int64_t)1 << 28)) return QCQPMI_EINVAL;
    if (!c->comm) return fail(c, QCQPMI_ESTATE, "comm_init has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t need = ((int64_t)(c->world + 1) * nbytes + 7) / 8;      // doubles: send area + receive area
    HIPCHK(c, c->d_comm_big.reserve(c->stream, (size_t)need, false));
    char *d_send = (char *)c->d_comm_big.p, *d_recv = d_send + nbytes;
    HIPCHK(c, hipMemcpyAsync(d_send, send, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, rccl()->AllGather(d_send, d_recv, (size_t)nbytes, ncclInt8, c->comm, c->stream));
    HIPCHK(c, hipMemcpyAsync(recv, d_recv, (size_t)nbytes * (size_t)c->world, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_comm_select_best(qcqpmi_ctx *c, double tol, int64_t index_offset, int64_t *best_global_index,
                            double *best_f0, double *best_maxviol, double *best_x) {
    if (!c) return QCQPMI_EINVAL;
    if (!c->comm) return fail(c, QCQPMI_ESTATE, "comm_init has not been called");
    int64_t li = -1;
    double lf = 0.0, lv = 0.0;
    int rc = qcqpmi_select_best(c, tol, &li, &lf, &lv, nullptr);
    if (rc) return rc;
    // key record: (bucket, f0, maxviol, global index) as 4 doubles (indices < 2^53 are exact)
    double rec[4] = {std::floor(lv / tol), lf, lv, (double)(index_offset + li)};
    if (!(lv == lv) || !(lf == lf) || li < 0) rec[0] = 9.0e18;
    const int W = c->world;
    double *d_send = c->d_comm, *d_recv = c->d_comm + 4, *d_x = c->d_comm + 4 + 4 * (size_t)W;
    HIPCHK(c, hipMemcpyAsync(d_send, rec, sizeof(rec), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, rccl()->AllGather(d_send, d_recv, 4, ncclDouble, c->comm, c->stream));
    std::vector<double> all((size_t)4 * W);
    HIPCHK(c, hipMemcpyAsync(all.data(), d_recv, all.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    int win = 0;
    for (int w = 1; w < W; w++) {
        const double *a = &all[(size_t)4 * w], *b = &all[(size_t)4 * win];
        if (a[0] < b[0] || (a[0] == b[0] && (a[1] < b[1] || (a[1] == b[1] && a[3] < b[3])))) win = w;
    }
    if (c->rank == win && li >= 0) {
        const double *src = c->X + (li >> 4) * c->n16 * 16 + (li & 15);
        HIPCHK(c, hipMemcpy2DAsync(d_x, sizeof(double), src, 16 * sizeof(double), sizeof(double), (size_t)c->n,
                                   hipMemcpyDeviceToDevice, c->stream));
    }
    NCCLCHK(c, rccl()->Broadcast(d_x, d_x, (size_t)c->n, ncclDouble, win, c->comm, c->stream));
    if (best_x) HIPCHK(c, hipMemcpyAsync(best_x, d_x, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    if (best_global_index) *best_global_index = (int64_t)all[(size_t)4 * win + 3];
    if (best_f0) *best_f0 = all[(size_t)4 * win + 1];
    if (best_maxviol) *best_maxviol = all[(size_t)4 * win + 2];
    return 0;
}

}  // extern "C"
