// host_comm.hip -- the multi-GPU layer of the C-ABI (include/zvx.h: zvx_comm_*): RCCL through dlopen, gathers on a stream of their own.
// The only unit that includes <rccl/rccl.h>.
#include "zvx_host.h"

#include <dlfcn.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is dlopen'ed by zvx_comm_* (single-GPU use never loads it)

extern "C" {
// ---- RCCL, resolved at run time ----------------------------------------------------------------------------------
extern "C++" {
namespace {
struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;            // optional (zvx_comm_info)
    decltype(&ncclGetVersion) GetVersion = nullptr;
};
Rccl& rccl() {
    static Rccl r;
    if (r.h) return r;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (r.h) break; }
    if (!r.h) fail(ZVX_E_HIP, "cannot load librccl.so (%s): multi-GPU needs RCCL", dlerror());
#define ZVX_SYM(f) do { r.f = (decltype(r.f))dlsym(r.h, "nccl" #f); if (!r.f) fail(ZVX_E_HIP, "librccl.so lacks nccl" #f); } while (0)
    ZVX_SYM(GetUniqueId); ZVX_SYM(CommInitRank); ZVX_SYM(CommDestroy); ZVX_SYM(Send); ZVX_SYM(Recv); ZVX_SYM(GroupStart); ZVX_SYM(GroupEnd);
    ZVX_SYM(AllReduce); ZVX_SYM(GetErrorString);
#undef ZVX_SYM
    r.CommCount = (decltype(r.CommCount))dlsym(r.h, "ncclCommCount");
    r.GetVersion = (decltype(r.GetVersion))dlsym(r.h, "ncclGetVersion");
    return r;
}
#define NCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) fail(ZVX_E_HIP, "%s failed: %s (%s:%d)", #x, rccl().GetErrorString(r_), __FILE__, __LINE__); } while (0)
}  // namespace
}  // extern "C++"

zvx_status zvx_comm_unique_id(void* id_out) {
    static_assert(sizeof(ncclUniqueId) == ZVX_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id_out) return ZVX_E_INVALID;
    try {
        ncclUniqueId id;
        NCCLCHK(rccl().GetUniqueId(&id));
        memcpy(id_out, &id, sizeof id);
        return ZVX_OK;
    } catch (const ZvxError& e) { g_create_error = e.what(); return e.code; }
}

zvx_status zvx_comm_init(zvx_ctx* c, const void* id, int rank, int world) {
    return guarded(c, [&] {
        if (world < 1 || rank < 0 || rank >= world) fail(ZVX_E_INVALID, "zvx_comm_init: rank %d of %d", rank, world);
        if (c->comm || c->comm_stream) fail(ZVX_E_STATE, "zvx_comm_init: communicator already initialised");
        HIPCHK(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->ev_compute, hipEventDisableTiming));
        c->rank = rank; c->world = world;
        if (world > 1 || id) {                              // world == 1 with an id: a real one-rank communicator (self-test of the RCCL path)
            if (!id) fail(ZVX_E_INVALID, "zvx_comm_init: id is NULL");
            ncclUniqueId uid;
            memcpy(&uid, id, sizeof uid);
            NCCLCHK(rccl().CommInitRank(&c->comm, world, uid, rank));
        }
    });
}

zvx_status zvx_comm_gather(zvx_ctx* c, const void* local, size_t bytes, void* recv, int root, int flags) {
    return guarded(c, [&] {
        if (!c->comm_stream) fail(ZVX_E_STATE, "zvx_comm_gather: call zvx_comm_init first");
        if (!local || root < 0 || root >= c->world || (c->rank == root && !recv)) fail(ZVX_E_INVALID, "zvx_comm_gather: bad arguments");
        // the communication stream picks up after everything issued so far on the compute stream
        HIPCHK(hipEventRecord(c->ev_compute, c->stream));
        HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_compute, 0));
        if (c->comm && c->world == 1) {                     // one-rank communicator: the root's row travels through RCCL too
            Rccl& r = rccl();
            NCCLCHK(r.GroupStart());
            NCCLCHK(r.Send(local, bytes, ncclInt8, 0, c->comm, c->comm_stream));
            NCCLCHK(r.Recv(recv, bytes, ncclInt8, 0, c->comm, c->comm_stream));
            NCCLCHK(r.GroupEnd());
        } else if (c->rank == root)
            HIPCHK(hipMemcpyAsync((char*)recv + (size_t)root * bytes, local, bytes, hipMemcpyDeviceToDevice, c->comm_stream));
        if (c->world > 1) {
            Rccl& r = rccl();
            NCCLCHK(r.GroupStart());
            if (c->rank == root) {
                for (int p = 0; p < c->world; p++)
                    if (p != root) NCCLCHK(r.Recv((char*)recv + (size_t)p * bytes, bytes, ncclInt8, p, c->comm, c->comm_stream));
            } else {
                NCCLCHK(r.Send(local, bytes, ncclInt8, root, c->comm, c->comm_stream));
            }
            NCCLCHK(r.GroupEnd());
        }
        // later writers of `local` (the vocoder of a coming call) queue behind this event on the device
        hipEvent_t& ev = c->gather_fence[local];
        if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(ev, c->comm_stream));
        if (!(flags & ZVX_NO_SYNC)) c->sync();
    });
}

zvx_status zvx_comm_max_f64(zvx_ctx* c, double* value) {
    return guarded(c, [&] {
        if (!c->comm_stream || !value) fail(ZVX_E_STATE, "zvx_comm_max_f64: call zvx_comm_init first");
        double* d = (double*)c->buf("comm.scalar", 64);      // (a first use zero-fills it on the compute stream: taken BEFORE the drain below,
        c->sync();                                           //  the communication stream must not see that fill land on top of its copy)
        if (!c->comm) return;
        HIPCHK(hipMemcpyAsync(d, value, sizeof(double), hipMemcpyHostToDevice, c->comm_stream));
        NCCLCHK(rccl().AllReduce(d, d, 1, ncclFloat64, ncclMax, c->comm, c->comm_stream));
        HIPCHK(hipMemcpyAsync(value, d, sizeof(double), hipMemcpyDeviceToHost, c->comm_stream));
        HIPCHK(hipStreamSynchronize(c->comm_stream));
    });
}

// Who is in the job, as seen by the communicator itself (bench.py puts it into the N > 1 JSON line so that the first multi-GPU
// run is self-diagnosing): out[0] = world of this context, out[1] = ncclCommCount, out[2] = ncclGetVersion code,
// out[3] = number of ranks that contributed to an all-reduce SUM of ones (a live data-path check), out[4 + r] = PCI address of
// rank r's device ((domain << 16) | (bus << 8) | (device << 3) | function), gathered with an all-reduce MAX over per-rank slots.
// Collective: every rank calls it.  Without a communicator (world 1, no id) only this rank's entries are filled.
zvx_status zvx_comm_info(zvx_ctx* c, int64_t* out, int n_out) {
    return guarded(c, [&] {
        if (!c->comm_stream || !out) fail(ZVX_E_STATE, "zvx_comm_info: call zvx_comm_init first");
        const int W = c->world;
        if (n_out < 4 + W) fail(ZVX_E_BUFFER, "zvx_comm_info: need %d entries", 4 + W);
        double* const d = (double*)c->buf("comm.info", (size_t)(W + 1) * 8);      // (allocated -- and zero-filled on the compute stream -- before the drain)
        c->sync();
        for (int i = 0; i < n_out; i++) out[i] = -1;
        out[0] = W;
        char bus[64] = {0};
        long pci = -1;
        if (hipDeviceGetPCIBusId(bus, sizeof bus, c->device) == hipSuccess) {
            unsigned dom = 0, b = 0, d = 0, f = 0;
            if (sscanf(bus, "%x:%x:%x.%x", &dom, &b, &d, &f) >= 3) pci = ((long)dom << 16) | ((long)b << 8) | ((long)d << 3) | f;
        }
        std::vector<double> v((size_t)W + 1, 0.0);
        v[0] = 1.0; v[1 + c->rank] = (double)(pci + 1);          // + 1: an address of 0 still reads as "present"
        if (c->comm) {
            Rccl& r = rccl();
            int n = -1, ver = -1;
            if (r.CommCount) NCCLCHK(r.CommCount(c->comm, &n));
            if (r.GetVersion) NCCLCHK(r.GetVersion(&ver));
            out[1] = n; out[2] = ver;
            HIPCHK(hipMemcpyAsync(d, v.data(), (size_t)(W + 1) * 8, hipMemcpyHostToDevice, c->comm_stream));
            NCCLCHK(r.AllReduce(d, d, 1, ncclFloat64, ncclSum, c->comm, c->comm_stream));
            NCCLCHK(r.AllReduce(d + 1, d + 1, W, ncclFloat64, ncclMax, c->comm, c->comm_stream));
            HIPCHK(hipMemcpyAsync(v.data(), d, (size_t)(W + 1) * 8, hipMemcpyDeviceToHost, c->comm_stream));
            HIPCHK(hipStreamSynchronize(c->comm_stream));
        }
        out[3] = (int64_t)(v[0] + 0.5);
        for (int r = 0; r < W; r++) out[4 + r] = (int64_t)v[1 + r] - 1;
    });
}

zvx_status zvx_comm_barrier(zvx_ctx* c) {
    double one = 1.0;
    return zvx_comm_max_f64(c, &one);
}

void zvx_comm_destroy(zvx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    if (c->comm) { (void)rccl().CommDestroy(c->comm); c->comm = nullptr; }
    for (auto& kv : c->gather_fence) if (kv.second) (void)hipEventDestroy(kv.second);
    c->gather_fence.clear();
    if (c->ev_compute) { (void)hipEventDestroy(c->ev_compute); c->ev_compute = nullptr; }
    if (c->copy_is_comm) { c->copy_stream = nullptr; c->copy_is_comm = false; }      // (host deliveries rode this stream: the next one creates its own)
    if (c->comm_stream) { (void)hipStreamDestroy(c->comm_stream); c->comm_stream = nullptr; }
    c->world = 1; c->rank = 0;
}

}  // extern "C"
