// coala_comm.cpp -- the owner-partitioned fetch as ONE native call, split-phase and overlapped on two HIP streams:
//
//   caller's stream : route -> counts all-to-all -> [the one host read] -> ids all-to-all-v -> probe (hits copied; the
//                     requester's OWN shard written straight into `out`) -> fill round 0 -> fill round 1 ... -> un-permute 0, 1 ...
//   comm stream     :                                   wait fill 0 -> rows round 0 -> wait fill 1 -> rows round 1 ...
//
// Round k ships the k-th slice of EVERY peer's segment (xGMI is point-to-point: an all-to-all is bound by its busiest link,
// so every round keeps all links loaded), while the PCIe cold fill of the next slice runs beside it.  Own-shard rows never
// enter the exchange or a staging buffer.  One host synchronisation per minibatch (the 2G counts).
//
// Replaces, fused (paths relative to /root/reference): SSD_GNN_NVSHMEM_Cache::send_requests + read_feature
// (COALA_GNN_Modules/ssd_gnn_cache.cuh:111-174: N x 2 one-sided 8-byte puts, 3 nvshmem_barrier_all, N warp-level row puts,
// peers served one by one on G streams :132-174) and the "nccl" orchestration in
// COALA-GNN-Setup/COALA_GNN/COALA_GNN_Manager.py:143-211 (full-capacity all_to_all of ids, G(G-1) serial send/recv of rows,
// the `j == i` local copy :195-199).
//
// Two transports behind one interface: RCCL (one process per GPU, grouped ncclSend/ncclRecv drive every direct xGMI link at
// once) and an in-process one (G ranks = G host threads of one process, device-to-device copies ordered by events) used by
// single-process drivers and by the parity tests, which run the very same orchestration with G logical ranks on one GPU.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/coala_hip.h"
#include "coala_internal.h"

#define fail coala_fail_
#define HIPCHK COALA_HIPCHK
#define NCCLCHK(expr)                                                                                                   \
    do {                                                                                                                \
        ncclResult_t r_ = (expr);                                                                                       \
        if (r_ != ncclSuccess) return fail(COALA_ECOMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

namespace {

constexpr int kMaxRounds = 8;

struct Transport {
    int rank = 0, nranks = 1;
    // coala_comm_set_self_loopback: a rank's OWN segment goes through the transport's send/recv path like a peer's (diagnostics)
    bool self_loopback = false;
    virtual ~Transport() {}
    // recv[p] = element [me] of rank p's send (one int64 per peer, self included)
    virtual int all_to_all_i64(const int64_t* send_dev, int64_t* recv_dev, hipStream_t st) = 0;
    // counts / displacements in elements of elem_bytes bytes; the self segment moves only when include_self
    virtual int all_to_all_v(const void* send, const size_t* scnt, const size_t* sdis, void* recv, const size_t* rcnt,
                             const size_t* rdis, size_t elem_bytes, bool include_self, hipStream_t st) = 0;
    // make the peers fail instead of hang after a local error between collectives; the transport is unusable afterwards
    virtual void abort() = 0;
    // ranks as the transport itself counts them (not the number it was told at creation); negative on failure
    virtual int size() = 0;
};

// ------------------------------------------------------------------------------------------------------------ RCCL
struct RcclTransport : Transport {
    ncclComm_t comm = nullptr;
    ~RcclTransport() override {
        if (comm) (void)ncclCommDestroy(comm);
    }
    int all_to_all_i64(const int64_t* send_dev, int64_t* recv_dev, hipStream_t st) override {
        NCCLCHK(ncclAllToAll(send_dev, recv_dev, 1, ncclInt64, comm, st));
        return COALA_OK;
    }
    int all_to_all_v(const void* send, const size_t* scnt, const size_t* sdis, void* recv, const size_t* rcnt, const size_t* rdis,
                     size_t elem_bytes, bool include_self, hipStream_t st) override {
        const ncclDataType_t dt = (elem_bytes % 8 == 0) ? ncclInt64 : ncclFloat32;
        const size_t per = (elem_bytes % 8 == 0) ? elem_bytes / 8 : elem_bytes / 4;
        const bool self_by_rccl = include_self && self_loopback; // ncclSend + ncclRecv to oneself inside the group call: legal, and a local copy inside RCCL
        if (include_self && scnt[rank] && !self_by_rccl)
            HIPCHK(hipMemcpyAsync((char*)recv + rdis[rank] * elem_bytes, (const char*)send + sdis[rank] * elem_bytes, scnt[rank] * elem_bytes,
                                  hipMemcpyDeviceToDevice, st));
        NCCLCHK(ncclGroupStart());
        for (int p = 0; p < nranks; ++p) {
            if (p == rank && !self_by_rccl) continue;
            if (scnt[p]) NCCLCHK(ncclSend((const char*)send + sdis[p] * elem_bytes, scnt[p] * per, dt, p, comm, st));
            if (rcnt[p]) NCCLCHK(ncclRecv((char*)recv + rdis[p] * elem_bytes, rcnt[p] * per, dt, p, comm, st));
        }
        NCCLCHK(ncclGroupEnd());
        return COALA_OK;
    }
    void abort() override {
        if (comm) (void)ncclCommAbort(comm);
        comm = nullptr;
    }
    int size() override {
        if (!comm) return fail(COALA_ECOMM, "the RCCL communicator was aborted");
        int n = -1;
        NCCLCHK(ncclCommCount(comm, &n));
        return n;
    }
};

} // namespace

// ------------------------------------------------------------------------------------------------------------ in-process
struct coala_comm_group {
    int nranks = 0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t phase = 0;
    bool aborted = false;
    int attached = 0;
    int timeout_s = 120; // COALA_INPROC_TIMEOUT_S
    struct Slot {
        const void* send = nullptr;
        const size_t* scnt = nullptr;
        const size_t* sdis = nullptr;
        hipEvent_t ready = nullptr, done = nullptr;
        int device = -1; // the device this rank's buffers live on
    };
    std::vector<Slot> slot;
    // peer_state[a * 64 + b]: may a kernel on device a read device b's memory?  0 unknown, 1 yes (same device, or peer access
    // enabled and verified), 2 no (the runtime's copy engine moves the segment instead)
    std::vector<unsigned char> peer_state = std::vector<unsigned char>(64 * 64, 0);

    int barrier() { // -> 0, or -1 when the group was aborted
        std::unique_lock<std::mutex> lk(m);
        if (aborted) return -1;
        const uint64_t my = phase;
        if (++arrived == nranks) {
            arrived = 0;
            ++phase;
            cv.notify_all();
            return 0;
        }
        // a peer that never arrives (it failed before its collective call, or its thread died) must not hang the others forever
        if (!cv.wait_for(lk, std::chrono::seconds(timeout_s), [&] { return phase != my || aborted; })) {
            aborted = true;
            cv.notify_all();
        }
        return aborted ? -1 : 0;
    }
    void abort() {
        std::lock_guard<std::mutex> lk(m);
        aborted = true;
        cv.notify_all();
    }
};

namespace {

// Device-to-device segment copy of the in-process transport.  hipMemcpyAsync between two buffers of ONE device goes through a DMA
// engine at ~26 GB/s on this platform (8 logical ranks x 0.9 GB of rows per step of the configs[4] probe: 270 ms); a plain kernel
// moves the same bytes at HBM speed.  16-B accesses when both ends are 16-B aligned, bytes otherwise.
__global__ __launch_bounds__(256) void inproc_copy_kernel(char* __restrict__ dst, const char* __restrict__ src, size_t bytes) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (size_t)gridDim.x * blockDim.x;
    if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0) {
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const size_t n16 = bytes / 16;
        for (size_t i = tid; i < n16; i += nthreads) reinterpret_cast<u32x4*>(dst)[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + i);
        for (size_t i = n16 * 16 + tid; i < bytes; i += nthreads) dst[i] = src[i];
    } else {
        for (size_t i = tid; i < bytes; i += nthreads) dst[i] = src[i];
    }
}

// kernel_ok: the source is on this device, or on a peer whose memory this device has mapped (peer_readable below).  Otherwise --
// and for small segments (ids, counts) -- the runtime's copy, which needs no peer mapping.
int inproc_copy(void* dst, const void* src, size_t bytes, hipStream_t st, bool kernel_ok) {
    if (bytes < (64u << 10) || !kernel_ok) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st));
        return COALA_OK;
    }
    const size_t blocks = (bytes / 16 + 256 * 8 - 1) / (256 * 8);
    hipLaunchKernelGGL(inproc_copy_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, (char*)dst, (const char*)src, bytes);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

// May a kernel running on device `mine` read memory of device `theirs`?  Decided once per ordered pair (under the group's mutex):
// hipDeviceCanAccessPeer + hipDeviceEnablePeerAccess; a pair without peer access is served by hipMemcpyAsync.
bool peer_readable(coala_comm_group* g, int mine, int theirs) {
    if (mine == theirs) return true;
    if (mine < 0 || theirs < 0 || mine >= 64 || theirs >= 64) return false;
    std::lock_guard<std::mutex> lk(g->m);
    unsigned char& st = g->peer_state[(size_t)mine * 64 + theirs];
    if (st == 0) {
        int can = 0;
        st = 2;
        if (hipDeviceCanAccessPeer(&can, mine, theirs) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(theirs, 0); // (the calling thread's current device is `mine`)
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) st = 1;
        }
        (void)hipGetLastError();
    }
    return st == 1;
}

struct InprocTransport : Transport {
    coala_comm_group* g = nullptr;
    int device = -1;
    int all_to_all_v(const void* send, const size_t* scnt, const size_t* sdis, void* recv, const size_t* rcnt, const size_t* rdis,
                     size_t elem_bytes, bool include_self, hipStream_t st) override {
        auto& me = g->slot[rank];
        me.send = send;
        me.scnt = scnt;
        me.sdis = sdis;
        HIPCHK(hipEventRecord(me.ready, st)); // my send buffer is complete at this point of my stream
        if (g->barrier()) return fail(COALA_ECOMM, "in-process group aborted (a peer failed or did not arrive in time)");
        for (int p = 0; p < nranks; ++p) {
            if (p == rank && !include_self) continue;
            const auto& peer = g->slot[p];
            if (peer.scnt[rank] != rcnt[p]) {
                g->abort();
                return fail(COALA_ECOMM, "in-process exchange: rank %d sends %zu elements to rank %d, which expects %zu", p, peer.scnt[rank], rank, rcnt[p]);
            }
            if (!rcnt[p]) continue;
            if (p != rank) HIPCHK(hipStreamWaitEvent(st, peer.ready, 0));
            if (int rc = inproc_copy((char*)recv + rdis[p] * elem_bytes, (const char*)peer.send + peer.sdis[rank] * elem_bytes, rcnt[p] * elem_bytes, st,
                                     peer_readable(g, device, peer.device)))
                return rc;
        }
        HIPCHK(hipEventRecord(me.done, st)); // I have pulled what I need from everybody
        if (g->barrier()) return fail(COALA_ECOMM, "in-process group aborted (a peer failed or did not arrive in time)");
        for (int p = 0; p < nranks; ++p) // nobody reuses its send buffer before every peer has pulled from it
            if (p != rank) HIPCHK(hipStreamWaitEvent(st, g->slot[p].done, 0));
        // no third barrier: a peer that races ahead rewrites its slot only before the NEXT exchange's first barrier, which this
        // rank has to reach too; send / counts are read above, before the second barrier
        return COALA_OK;
    }
    int all_to_all_i64(const int64_t* send_dev, int64_t* recv_dev, hipStream_t st) override {
        std::vector<size_t> one((size_t)nranks, 1), dis((size_t)nranks);
        for (int p = 0; p < nranks; ++p) dis[p] = (size_t)p;
        return all_to_all_v(send_dev, one.data(), dis.data(), recv_dev, one.data(), dis.data(), sizeof(int64_t), true, st);
    }
    void abort() override { g->abort(); }
    int size() override { return g->nranks; }
};

int grow_workspace(void** p, uint64_t* cap, uint64_t need, size_t elem, hipStream_t st) {
    if (need <= *cap) return COALA_OK;
    HIPCHK(hipStreamSynchronize(st));
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    uint64_t c = 4096;
    while (c < need) c *= 2;
    if (c - need > (c >> 2) && need > (1ull << 20)) c = need + (need >> 3); // large buffers: 12 % head room instead of up to 100 %
    if (hipMalloc(p, c * elem) != hipSuccess) {
        (void)hipGetLastError();
        return fail(COALA_ENOMEM, "hipMalloc(%llu) failed for the exchange workspace", (unsigned long long)(c * elem));
    }
    *cap = c;
    return COALA_OK;
}

struct Range { size_t begin, end; };

// Who sends how many ids to whom in one fetch, and how every segment is cut into K rounds.  Two sides: kServed = the batch this rank serves as
// an owner, the segments it received in source-rank order (positions of recv_ids / rows_send); kRequested = this rank's own batch in bucket
// order (positions of node / rows_recv).
struct Segments {
    enum Side { kServed, kRequested };
    int me = 0, K = 1;
    bool loop = false; // self-loopback: no own-shard bypass, the own segment is a peer's like any other
    std::vector<size_t> scnt, sdis, rcnt, rdis; // per peer: ids this rank sends to it / receives from it, and where its segment starts
    size_t total_send = 0, total_recv = 0;
    // the own segment never enters the exchange: its rows go straight from the probe and the fill into `out`
    bool bypassed(int p) const { return p == me && !loop; }
    // Round k of peer p's segment on either side.  A bypassed own segment is empty in every round of the exchange; `fill` asks for what the
    // cold fill of round k covers instead, where it is whole in the last round: nobody waits for it on a link.  The same rule as
    // _round_slices (COALA_GNN_Manager.py), which the torch exchange cuts its rounds with, and it has to stay so.
    Range slice(Side side, int p, int k, bool fill = false) const {
        const size_t cnt = side == kServed ? rcnt[p] : scnt[p], dis = side == kServed ? rdis[p] : sdis[p];
        const size_t a = dis + cnt * (size_t)k / (size_t)K, b = dis + cnt * (size_t)(k + 1) / (size_t)K;
        if (!bypassed(p)) return {a, b};
        return (fill && k == K - 1) ? Range{dis, dis + cnt} : Range{a, a};
    }
};

} // namespace

struct coala_comm {
    Transport* tr = nullptr;
    int rank = 0, nranks = 1, device = 0;
    int rounds = 2;                 // row-exchange rounds per fetch (COALA_EXCHANGE_ROUNDS; coala_comm_set_rounds)
    hipStream_t cs = nullptr;       // the communication stream of this rank
    hipEvent_t ev_fill[kMaxRounds] = {}, ev_x[kMaxRounds] = {};
    // workspace (device), grown on demand, persistent across steps
    int64_t *node = nullptr, *map = nullptr, *recv_ids = nullptr;
    uint64_t node_cap = 0, map_cap = 0, recv_cap = 0;
    float *rows_send = nullptr, *rows_recv = nullptr;
    uint64_t rows_send_cap = 0, rows_recv_cap = 0; // in floats
    int64_t* counts_dev = nullptr;                 // [3G+1]: send counts, recv counts, offsets
    int64_t* counts_host = nullptr;                // pinned [2G]
    Segments seg;                                  // the plan of the last fetch (its counts: coala_comm_last_counts)
    // profiling of the row exchange (coala_comm_profile)
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_live;
    EventPool prof_pool;
    coala_comm_profile_t prof{};
    bool broken = false;
    // coala_comm_fetch_events: begin / end events of a bucketed fetch without packets of their own on the caller's stream; a ring of triples
    // (begin on the probe's launch, end on the last fill launch of the caller's stream, end behind the last row round on the communicator's stream)
    int fetch_events = 0;           // 0 off, 1 end events only, 2 begin event too (coala_comm_fetch_events)
    static constexpr int kFetchRing = 2048;
    std::vector<hipEvent_t> fev;    // [3 * kFetchRing], created on first use
    uint64_t fev_calls = 0;
    hipEvent_t last_ev[3] = {nullptr, nullptr, nullptr};
    // count exchanges issued ahead of their fetch (coala_comm_counts_begin): ring of device [2G] + pinned [2G] + event
    static constexpr int kCountsRing = COALA_COUNTS_RING;
    int64_t* ahead_dev = nullptr;   // [kCountsRing][2G]
    int64_t* ahead_host = nullptr;  // pinned [kCountsRing][2G]
    hipEvent_t ahead_ev[kCountsRing] = {};
    uint64_t ahead_calls = 0;
    // The workspaces (recv_ids, rows_send, node/map) are ordered by the stream the fetches are enqueued on.  A caller that moves to
    // another stream keeps that order: the new stream first waits (no host wait) for what the previous fetch enqueued on the old
    // one -- the cache handle's rule (StreamOrder, coala_internal.h).
    StreamOrder order;
};

namespace {

// How both constructors begin: the handle around its transport (null, both freed, when the host is out of memory) ...
coala_comm* new_comm(Transport* t, int rank, int nranks, int device) {
    coala_comm* c = new (std::nothrow) coala_comm();
    if (!c || !t) {
        delete c;
        delete t;
        return nullptr;
    }
    c->tr = t;
    c->device = device;
    c->rank = t->rank = rank;
    c->nranks = t->nranks = nranks;
    return c;
}

// ... and what they give it once the transport stands: stream, events, workspaces.
int equip(coala_comm* c) {
    if (const char* e = getenv("COALA_EXCHANGE_ROUNDS")) {
        const int r = atoi(e);
        if (r >= 1 && r <= kMaxRounds) c->rounds = r;
    }
    // The communication stream gets the highest stream priority: HIP keeps priority levels on separate hardware queues, so the row
    // exchange can never be queued behind the cold fill it is meant to run beside (with equal priorities the streams of a process
    // share GPU_MAX_HW_QUEUES = 4 queues in creation order), and its few workgroups are scheduled ahead of the fill's.
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess ||
        hipStreamCreateWithPriority(&c->cs, hipStreamNonBlocking, prio_greatest) != hipSuccess) {
        (void)hipGetLastError();
        c->cs = nullptr;
        if (hipStreamCreateWithFlags(&c->cs, hipStreamNonBlocking) != hipSuccess) return fail(COALA_EHIP, "hipStreamCreate failed");
    }
    for (int k = 0; k < 2 * kMaxRounds + coala_comm::kCountsRing; ++k) {
        hipEvent_t* e = k < kMaxRounds ? &c->ev_fill[k] : k < 2 * kMaxRounds ? &c->ev_x[k - kMaxRounds] : &c->ahead_ev[k - 2 * kMaxRounds];
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return fail(COALA_EHIP, "hipEventCreate failed");
    }
    for (auto* v : {&c->seg.scnt, &c->seg.sdis, &c->seg.rcnt, &c->seg.rdis}) v->assign(c->nranks, 0);
    const size_t ring_words = (size_t)coala_comm::kCountsRing * 2 * (size_t)c->nranks;
    if (hipMalloc((void**)&c->counts_dev, (3 * (size_t)c->nranks + 1) * sizeof(int64_t)) != hipSuccess ||
        hipHostMalloc((void**)&c->counts_host, 2 * (size_t)c->nranks * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void**)&c->ahead_dev, ring_words * sizeof(int64_t)) != hipSuccess || hipHostMalloc((void**)&c->ahead_host, ring_words * sizeof(int64_t)) != hipSuccess)
        return fail(COALA_ENOMEM, "communicator workspace allocation failed");
    return COALA_OK;
}

void drain_profile(coala_comm* c) {
    for (auto& p : c->prof_live) {
        float ms = 0.f;
        if (hipEventSynchronize(p.second) == hipSuccess && hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) c->prof.rows_ms += ms;
        c->prof_pool.give(p.first);
        c->prof_pool.give(p.second);
    }
    c->prof_live.clear();
}

// A communicator that went through abandon() takes no further calls.
int refuse_abandoned(const coala_comm* c) {
    return c->broken ? fail(COALA_ECOMM, "this communicator failed in an earlier fetch and was aborted: destroy it") : COALA_OK;
}

// The one way out of a call that fails locally once its peers may be inside (or about to enter) a collective this rank will not join: the
// transport is aborted, so that they error out instead of waiting for this rank.  -> code
int abandon(coala_comm* c, int code) {
    c->broken = true;
    c->tr->abort();
    return code;
}

// Slot of the counts-ahead ring that ticket `t` uses: device [2G] (send counts, recv counts), its pinned host copy, the event behind that copy.
struct CountsSlot { int64_t *dev, *host; hipEvent_t ev; };
CountsSlot counts_slot(const coala_comm* c, uint64_t t) {
    const size_t s = (size_t)(t % coala_comm::kCountsRing), words = s * 2 * (size_t)c->nranks;
    return {c->ahead_dev + words, c->ahead_host + words, c->ahead_ev[s]};
}

// Slot of the fetch-event ring that call number `call` uses: {begin, end on the caller's stream, end on the communicator's}, created on first
// use; nullptr when that fails.
hipEvent_t* fetch_event_slot(coala_comm* c, uint64_t call) {
    if (c->fev.empty()) c->fev.assign(3 * (size_t)coala_comm::kFetchRing, nullptr);
    hipEvent_t* slot = c->fev.data() + 3 * (size_t)(call % coala_comm::kFetchRing);
    for (int k = 0; k < 3; ++k)
        if (!slot[k] && hipEventCreate(&slot[k]) != hipSuccess) return nullptr;
    return slot;
}

// ------------------------------------------------------------------------------------------------------------ the fetch
struct FetchCall {
    coala_cache_t* h; coala_comm* c; float* out; const int64_t* idx; int64_t n; hipStream_t st;
    // device [G], not null: idx is already bucketed by owner -- the batch in bucket order is idx itself, the map is the identity, the rows of every
    // peer are received straight into `out` and nothing is un-permuted.  Null: route here, into the communicator's node / map / rows_recv.
    const int64_t* bucket_counts_dev = nullptr;
    // host [2G], not null: the counts were exchanged ahead (coala_comm_counts_begin) -- no count exchange, no host synchronisation in this call
    const int64_t* counts_host = nullptr;
    // check_call: what the steps share
    int G = 0, me = 0, K = 1; // K: row-exchange rounds of this fetch
    int64_t dim = 0;
    bool bucketed = false, loop = false, exchange_rows = false;
    // Events of this fetch.  Every hipEventRecord on the caller's stream is one more barrier packet between the kernels of a saturated stream
    // (6-12 us each: DESIGN.md section 6), so whatever can ride ON a launch does: the hand-over events of the fill rounds always, and -- opt-in,
    // bucketed fetches: coala_comm_fetch_events -- the begin / end events a caller needs for timing and for its consumer's stream.
    hipEvent_t ev_begin = nullptr, ev_end_st = nullptr, ev_end_cs = nullptr; // choose_events; ev_end_st set = this fetch hands events out
    hipEvent_t fill_evs[kMaxRounds] = {}, x_evs[kMaxRounds] = {}; // what round k of the rows waits for / what it leaves behind
};

// 1. Everything that can be refused without touching the device.
int check_call(FetchCall& f) {
    if (!f.h || !f.c) return fail(COALA_EINVAL, "null handle");
    coala_comm* c = f.c;
    c->last_ev[0] = c->last_ev[1] = c->last_ev[2] = nullptr;
    if (int rc = refuse_abandoned(c)) return rc;
    if (f.n < 0 || f.n > 0x7FFFFFFFll || (f.n > 0 && (!f.out || !f.idx))) return fail(COALA_EINVAL, "bad batch");
    coala_cache_geometry_t geo;
    if (int rc = coala_cache_geometry(f.h, &geo)) return rc;
    f.G = c->nranks, f.me = c->rank, f.dim = coala_cache_row_dim(f.h);
    f.bucketed = f.bucket_counts_dev != nullptr;
    f.loop = c->tr->self_loopback;
    f.exchange_rows = f.G > 1 || f.loop; // a lone rank without loopback has nobody to exchange rows with: one fill round, no row rounds
    f.K = f.exchange_rows ? c->rounds : 1;
    return COALA_OK;
}

// 2. Behind whatever the previous fetch enqueued, on whichever stream; workspaces for a batch of n.
int follow_and_presize(FetchCall& f) {
    coala_comm* c = f.c;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = c->order.follow(f.st)) return rc;
    const uint64_t nb = (uint64_t)(f.n > 0 ? f.n : 1), dim = (uint64_t)f.dim;
    if (!f.bucketed) {
        if (int rc = grow_workspace((void**)&c->node, &c->node_cap, nb, sizeof(int64_t), f.st)) return rc;
        if (int rc = grow_workspace((void**)&c->map, &c->map_cap, nb, sizeof(int64_t), f.st)) return rc;
        if (int rc = grow_workspace((void**)&c->rows_recv, &c->rows_recv_cap, nb * dim, sizeof(float), f.st)) return rc;
    }
    // the usual step receives about as many ids as it sends: pre-size the owner-side buffers too, so that the grow after the
    // counts exchange (the one allocation that sits between collectives) only happens for skewed batches
    if (int rc = grow_workspace((void**)&c->recv_ids, &c->recv_cap, nb + (nb >> 2), sizeof(int64_t), f.st)) return rc;
    return grow_workspace((void**)&c->rows_send, &c->rows_send_cap, (nb + (nb >> 2)) * dim, sizeof(float), f.st);
}

// 3. Bucket by owner (stable), packed layout -- unless the sampler already delivered the ids that way.  counts_dev: [G] send counts, [G] recv
//    counts, [G+1] offsets.
int bucket_ids(FetchCall& f) {
    coala_comm* c = f.c;
    if (!f.bucketed) return coala_cache_route(f.h, f.idx, f.n, f.G, 0, c->node, c->map, c->counts_dev, c->counts_dev + 2 * f.G, f.st);
    if (!f.counts_host) HIPCHK(hipMemcpyAsync(c->counts_dev, f.bucket_counts_dev, (size_t)f.G * sizeof(int64_t), hipMemcpyDeviceToDevice, f.st));
    return COALA_OK;
}

// 4. Counts: every rank tells every owner how many ids follow; then the one host read of the step.
int exchange_counts(FetchCall& f) {
    coala_comm* c = f.c;
    if (f.counts_host) return COALA_OK;
    if (int rc = c->tr->all_to_all_i64(c->counts_dev, c->counts_dev + f.G, f.st)) return rc;
    if (hipMemcpyAsync(c->counts_host, c->counts_dev, 2 * (size_t)f.G * sizeof(int64_t), hipMemcpyDeviceToHost, f.st) != hipSuccess ||
        hipStreamSynchronize(f.st) != hipSuccess)
        return fail(COALA_EHIP, "reading the exchange counts failed: %s", hipGetErrorString(hipGetLastError()));
    f.counts_host = c->counts_host;
    return COALA_OK;
}

// 5. The segments of this fetch; the counts must add up to the batch.
int plan_segments(FetchCall& f) {
    Segments& s = f.c->seg;
    s.me = f.me, s.K = f.K, s.loop = f.loop, s.total_send = s.total_recv = 0;
    for (int p = 0; p < f.G; ++p) {
        s.scnt[p] = (size_t)f.counts_host[p], s.rcnt[p] = (size_t)f.counts_host[f.G + p];
        s.sdis[p] = s.total_send, s.rdis[p] = s.total_recv;
        s.total_send += s.scnt[p], s.total_recv += s.rcnt[p];
    }
    if ((int64_t)s.total_send != f.n)
        return fail(COALA_ECOMM, "%s %zu ids for a batch of %lld", f.bucketed ? "the bucket counts sum to" : "route produced", s.total_send, (long long)f.n);
    if (s.total_recv > 0x7FFFFFFFull) return fail(COALA_ECOMM, "%zu ids routed to one owner in one step", s.total_recv);
    return COALA_OK;
}

// 6. The owner-side buffers at their exact size (the one allocation between collectives: skewed batches only, see follow_and_presize).
int grow_owner_buffers(FetchCall& f) {
    coala_comm* c = f.c;
    const uint64_t tr = f.c->seg.total_recv ? f.c->seg.total_recv : 1;
    if (int rc = grow_workspace((void**)&c->recv_ids, &c->recv_cap, tr, sizeof(int64_t), f.st)) return rc;
    return grow_workspace((void**)&c->rows_send, &c->rows_send_cap, tr * (uint64_t)f.dim, sizeof(float), f.st);
}

// 7. Ids to their owners (exact sizes); the own bucket is a device copy.
int send_ids(FetchCall& f) {
    const Segments& s = f.c->seg;
    return f.c->tr->all_to_all_v(f.bucketed ? f.idx : f.c->node, s.scnt.data(), s.sdis.data(), f.c->recv_ids, s.rcnt.data(), s.rdis.data(), sizeof(int64_t), true, f.st);
}

// 8. The begin / end events this fetch hands out, when the caller asked for them.
int choose_events(FetchCall& f) {
    coala_comm* c = f.c;
    if (!c->fetch_events || !f.bucketed || f.n == 0) return COALA_OK;
    hipEvent_t* slot = fetch_event_slot(c, c->fev_calls);
    if (!slot) return fail(COALA_EHIP, "hipEventCreate failed");
    f.ev_begin = c->fetch_events >= 2 ? slot[0] : nullptr; // (an event on the probe's launch costs that launch ~5 us: only when asked for)
    f.ev_end_st = slot[1], f.ev_end_cs = slot[2];
    return COALA_OK;
}

// 9. Owner side: ONE batch = the concatenation in source-rank order (DESIGN.md "Determinism contract").  Probe all of it; the own segment is
//    delivered straight to out[map[..]] -- it never sees rows_send, the exchange or rows_recv.  (Self-loopback, diagnostics: no own-shard bypass
//    -- the own segment is served, shipped and un-permuted like a peer's, so that a communicator of ONE rank drives every line of the row
//    exchange through the transport.)
int probe(FetchCall& f) {
    coala_comm* c = f.c;
    const Segments& s = c->seg;
    coala_row_redirect_t rd; // the own segment's rows, unless it takes the road of a peer's
    rd.begin = (int64_t)s.rdis[s.me];
    rd.end = rd.begin + (int64_t)(s.bypassed(s.me) ? s.rcnt[s.me] : 0);
    rd.out = f.bucketed ? f.out + s.sdis[s.me] * (size_t)f.dim : f.out; // bucketed: the own bucket sits at its offset, in order
    rd.row_map = f.bucketed ? nullptr : c->map + s.sdis[s.me];
    hipEvent_t rode = nullptr;
    if (int rc = coala_serve_probe_redirect_ev_(f.h, c->rows_send, c->recv_ids, (int64_t)s.total_recv, &rd, f.st, f.ev_begin, &rode)) return rc;
    if (f.ev_begin && rode != f.ev_begin && hipEventRecord(f.ev_begin, f.st) != hipSuccess) return fail(COALA_EHIP, "hipEventRecord failed");
    return COALA_OK;
}

// The event that round k's fill hands to the communicator's stream: the fetch's end event on the caller's stream in the last round, else the
// round's own when rows are exchanged at all.
hipEvent_t fill_event(const FetchCall& f, int k) {
    if (k == f.K - 1 && f.ev_end_st) return f.ev_end_st;
    return f.exchange_rows ? f.c->ev_fill[k] : nullptr;
}

// ... and what became of it: `rode` is the event that really rides on round k's last fill launch -- fill_event(k), or the one a profiling cache
// handle lends in its place, or none when the round launched nothing.  Recorded the plain way when nothing rode, or when the event is handed
// out to the caller and a borrowed one will not do.  -> fill_evs[k]
int hand_over_fill(FetchCall& f, int k, hipEvent_t rode) {
    const hipEvent_t ev = fill_event(f, k);
    const bool must_be_mine = ev && ev == f.ev_end_st;
    if (ev && (rode == nullptr || (must_be_mine && rode != ev)) && hipEventRecord(ev, f.st) != hipSuccess) return fail(COALA_EHIP, "hipEventRecord failed");
    f.fill_evs[k] = (rode && !must_be_mine) ? rode : ev;
    return COALA_OK;
}

// 10. Fill slice k of every peer's segment on the caller's stream; the row round k ships it on the communicator's stream while slice k+1
//     fills.  A round without rows to fill (this rank serves nothing, or a segment has fewer ids than rounds) still hands its event over:
//     the row rounds run all the same -- peers may owe this rank rows.
int fill_rounds(FetchCall& f) {
    const Segments& s = f.c->seg;
    std::vector<int64_t> fb(f.G), fe(f.G);
    for (int k = 0; k < f.K; ++k) {
        int nr = 0;
        for (int p = 0; p < f.G; ++p) {
            const Range r = s.slice(Segments::kServed, p, k, true);
            if (r.end > r.begin) { fb[nr] = (int64_t)r.begin; fe[nr] = (int64_t)r.end; ++nr; }
        }
        hipEvent_t rode = nullptr;
        int rc = nr ? coala_serve_fill_ranges_ev_(f.h, f.c->rows_send, f.c->recv_ids, (int64_t)s.total_recv, fb.data(), fe.data(), nr, f.st, fill_event(f, k), &rode) : COALA_OK;
        if (!rc) rc = hand_over_fill(f, k, rode);
        if (rc) return rc;
    }
    return COALA_OK;
}

// 11. Row round k on the communicator's stream, behind fill round k.  (coala_comm_profile: one event pair around all rounds.)
int row_rounds(FetchCall& f) {
    if (!f.exchange_rows) return COALA_OK;
    coala_comm* c = f.c;
    const Segments& s = f.c->seg;
    if (c->profile && c->prof_live.size() >= 4096) drain_profile(c);
    const hipEvent_t t0 = c->profile ? c->prof_pool.take() : nullptr, t1 = c->profile ? c->prof_pool.take() : nullptr;
    std::vector<size_t> xs_cnt(f.G), xs_dis(f.G), xr_cnt(f.G), xr_dis(f.G);
    float* rows_recv = f.bucketed ? f.out : c->rows_recv; // bucket order IS the caller's order
    for (int k = 0; k < f.K; ++k) {
        for (int p = 0; p < f.G; ++p) {
            const Range mine = s.slice(Segments::kServed, p, k), theirs = s.slice(Segments::kRequested, p, k); // what I serve to p, what p serves to me
            xs_cnt[p] = mine.end - mine.begin, xs_dis[p] = mine.begin;
            xr_cnt[p] = theirs.end - theirs.begin, xr_dis[p] = theirs.begin;
        }
        if (hipStreamWaitEvent(c->cs, f.fill_evs[k], 0) != hipSuccess) return fail(COALA_EHIP, "hipStreamWaitEvent failed");
        if (k == 0 && t0) (void)hipEventRecord(t0, c->cs);
        if (int rc = c->tr->all_to_all_v(c->rows_send, xs_cnt.data(), xs_dis.data(), rows_recv, xr_cnt.data(), xr_dis.data(), (size_t)f.dim * sizeof(float), f.loop, c->cs))
            return rc;
        f.x_evs[k] = (k == f.K - 1 && f.ev_end_cs) ? f.ev_end_cs : c->ev_x[k];
        if (hipEventRecord(f.x_evs[k], c->cs) != hipSuccess) return fail(COALA_EHIP, "hipEventRecord failed");
    }
    if (t0 && t1) {
        (void)hipEventRecord(t1, c->cs);
        c->prof_live.emplace_back(t0, t1);
        c->prof.calls++;
        c->prof.remote_rows_in += (uint64_t)(f.n - (int64_t)s.scnt[f.me]);
    }
    return COALA_OK;
}

// 12. Un-permute round by round as the rows arrive.  (Bucketed: nothing to un-permute, and the communicator's stream completes its rounds in
//     order -- the caller's stream waits for the last one only; the workspaces are safe to reuse behind that wait.)
int unpermute(FetchCall& f) {
    if (!f.exchange_rows) return COALA_OK;
    std::vector<int64_t> sb(f.G), se(f.G); // ranges of rows_recv that round k filled
    for (int k = f.bucketed ? f.K - 1 : 0; k < f.K; ++k) {
        if (hipStreamWaitEvent(f.st, f.x_evs[k], 0) != hipSuccess) return fail(COALA_EHIP, "hipStreamWaitEvent failed");
        if (f.bucketed) continue;
        for (int p = 0; p < f.G; ++p) {
            const Range r = f.c->seg.slice(Segments::kRequested, p, k);
            sb[p] = (int64_t)r.begin, se[p] = (int64_t)r.end;
        }
        if (int rc = coala_cache_scatter_ranges(f.h, f.out, f.c->rows_recv, f.c->map, sb.data(), se.data(), f.G, f.st)) return rc;
    }
    return COALA_OK;
}

// 13. What coala_comm_last_fetch_events hands out.
void publish_events(FetchCall& f) {
    if (!f.ev_end_st) return;
    f.c->last_ev[0] = f.ev_begin;
    f.c->last_ev[1] = f.ev_end_st;
    f.c->last_ev[2] = f.exchange_rows ? f.ev_end_cs : nullptr;
    f.c->fev_calls++;
}

int fetch(FetchCall& f) {
    // every check that can fail locally comes BEFORE the first collective: a rank that returns between collectives strands its peers
    if (int rc = check_call(f)) return rc;
    if (int rc = follow_and_presize(f)) return rc;
    if (int rc = bucket_ids(f)) return rc;
    // from here on a local failure aborts the transport so that the peers error out instead of waiting for this rank
    int (*const steps[])(FetchCall&) = {exchange_counts, plan_segments, grow_owner_buffers, send_ids, choose_events, probe, fill_rounds, row_rounds, unpermute};
    for (auto step : steps)
        if (int rc = step(f)) return abandon(f.c, rc);
    publish_events(f);
    return COALA_OK;
}

// How both constructors end: a communicator that cannot be equipped is destroyed.
int finish_create(coala_comm* c, coala_comm_t** out) {
    const int rc = equip(c);
    if (rc) coala_comm_destroy(c);
    else *out = c;
    return rc;
}

} // namespace

extern "C" {

int coala_comm_unique_id(void* out_id, size_t cap) {
    if (!out_id || cap < NCCL_UNIQUE_ID_BYTES) return fail(COALA_EINVAL, "id buffer must hold %d bytes", NCCL_UNIQUE_ID_BYTES);
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(out_id, &id, NCCL_UNIQUE_ID_BYTES);
    return COALA_OK;
}

int coala_comm_create(const void* id_bytes, int rank, int nranks, int device, coala_comm_t** out) {
    if (!id_bytes || !out || nranks < 1 || rank < 0 || rank >= nranks || nranks > 64) return fail(COALA_EINVAL, "bad communicator arguments");
    *out = nullptr;
    HIPCHK(hipSetDevice(device));
    RcclTransport* t = new (std::nothrow) RcclTransport();
    coala_comm* c = new_comm(t, rank, nranks, device);
    if (!c) return fail(COALA_ENOMEM, "out of host memory");
    ncclUniqueId id;
    memcpy(&id, id_bytes, NCCL_UNIQUE_ID_BYTES);
    ncclResult_t r = ncclCommInitRank(&t->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        coala_comm_destroy(c);
        return fail(COALA_ECOMM, "ncclCommInitRank failed: %s", ncclGetErrorString(r));
    }
    {   // what RCCL itself thinks this communicator is: it must agree with what the caller asked for
        int cnt = -1, urank = -1, dev = -1;
        if (ncclCommCount(t->comm, &cnt) != ncclSuccess || ncclCommUserRank(t->comm, &urank) != ncclSuccess ||
            ncclCommCuDevice(t->comm, &dev) != ncclSuccess || cnt != nranks || urank != rank || dev != device) {
            coala_comm_destroy(c);
            return fail(COALA_ECOMM, "RCCL reports %d ranks / rank %d / device %d for a communicator created as %d ranks / rank %d / device %d",
                        cnt, urank, dev, nranks, rank, device);
        }
    }
    return finish_create(c, out);
}

int coala_comm_group_create(int nranks, coala_comm_group_t** out) {
    if (!out || nranks < 1 || nranks > 64) return fail(COALA_EINVAL, "bad group size");
    coala_comm_group* g = new (std::nothrow) coala_comm_group();
    if (!g) return fail(COALA_ENOMEM, "out of host memory");
    g->nranks = nranks;
    g->slot.resize((size_t)nranks);
    if (const char* e = getenv("COALA_INPROC_TIMEOUT_S")) {
        const int t = atoi(e);
        if (t > 0) g->timeout_s = t;
    }
    *out = g;
    return COALA_OK;
}

int coala_comm_group_destroy(coala_comm_group_t* g) {
    if (!g) return COALA_OK;
    if (g->attached) return fail(COALA_EINVAL, "%d communicators of this group are still alive", g->attached);
    delete g;
    return COALA_OK;
}

int coala_comm_create_inproc(coala_comm_group_t* g, int rank, int device, coala_comm_t** out) {
    if (!g || !out || rank < 0 || rank >= g->nranks) return fail(COALA_EINVAL, "bad in-process communicator arguments");
    *out = nullptr;
    HIPCHK(hipSetDevice(device));
    InprocTransport* t = new (std::nothrow) InprocTransport();
    coala_comm* c = new_comm(t, rank, g->nranks, device);
    if (!c) return fail(COALA_ENOMEM, "out of host memory");
    t->g = g;
    t->device = device;
    auto& sl = g->slot[rank];
    sl.device = device;
    if (sl.ready || hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess) {
        delete c;
        delete t;
        return fail(COALA_EINVAL, "rank %d of the group is taken, or hipEventCreate failed", rank);
    }
    {
        std::lock_guard<std::mutex> lk(g->m);
        g->attached++;
    }
    return finish_create(c, out);
}

int coala_comm_destroy(coala_comm_t* c) {
    if (!c) return COALA_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    drain_profile(c); // (the pool's events, and the stream order's, go with the handle)
    if (auto* t = dynamic_cast<InprocTransport*>(c->tr)) {
        auto& sl = t->g->slot[t->rank];
        if (sl.ready) (void)hipEventDestroy(sl.ready);
        if (sl.done) (void)hipEventDestroy(sl.done);
        sl.ready = sl.done = nullptr;
        std::lock_guard<std::mutex> lk(t->g->m);
        t->g->attached--;
    }
    delete c->tr;
    if (c->cs) (void)hipStreamDestroy(c->cs);
    std::vector<hipEvent_t> evs(c->fev);
    for (auto* a : {c->ev_fill, c->ev_x}) evs.insert(evs.end(), a, a + kMaxRounds);
    evs.insert(evs.end(), c->ahead_ev, c->ahead_ev + coala_comm::kCountsRing);
    for (auto e : evs)
        if (e) (void)hipEventDestroy(e);
    if (c->ahead_host) (void)hipHostFree(c->ahead_host);
    void* dev[] = {c->node, c->map, c->recv_ids, c->rows_send, c->rows_recv, c->counts_dev, c->ahead_dev};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (c->counts_host) (void)hipHostFree(c->counts_host);
    delete c;
    return COALA_OK;
}

int coala_comm_size(const coala_comm_t* c) { return (c && c->tr) ? c->tr->size() : 0; }

int coala_comm_set_rounds(coala_comm_t* c, int rounds) {
    if (!c || rounds < 1 || rounds > kMaxRounds) return fail(COALA_EINVAL, "rounds must be 1..%d", kMaxRounds);
    c->rounds = rounds;
    return COALA_OK;
}

int coala_comm_get_rounds(const coala_comm_t* c) { return c ? c->rounds : 0; }

int coala_comm_fetch_events(coala_comm_t* c, int enable) {
    if (!c) return fail(COALA_EINVAL, "null communicator");
    if (enable < 0 || enable > 2) return fail(COALA_EINVAL, "enable must be 0, 1 or 2");
    c->fetch_events = enable;
    if (!c->fetch_events) c->last_ev[0] = c->last_ev[1] = c->last_ev[2] = nullptr;
    return COALA_OK;
}

int coala_comm_last_fetch_events(const coala_comm_t* c, void** begin_ev, void** end_ev_stream, void** end_ev_comm) {
    if (!c) return fail(COALA_EINVAL, "null communicator");
    if (begin_ev) *begin_ev = (void*)c->last_ev[0];
    if (end_ev_stream) *end_ev_stream = (void*)c->last_ev[1];
    if (end_ev_comm) *end_ev_comm = (void*)c->last_ev[2];
    return COALA_OK;
}

int coala_comm_set_self_loopback(coala_comm_t* c, int on) {
    if (!c || !c->tr) return fail(COALA_EINVAL, "null communicator");
    c->tr->self_loopback = on != 0;
    return COALA_OK;
}

int coala_comm_last_counts(const coala_comm_t* c, int64_t* send, int64_t* recv) {
    if (!c) return fail(COALA_EINVAL, "null communicator");
    for (int p = 0; p < c->nranks; ++p) {
        if (send) send[p] = (int64_t)c->seg.scnt[p];
        if (recv) recv[p] = (int64_t)c->seg.rcnt[p];
    }
    return COALA_OK;
}

int coala_comm_profile(coala_comm_t* c, int enable, coala_comm_profile_t* out, int reset) {
    if (!c) return fail(COALA_EINVAL, "null communicator");
    HIPCHK(hipSetDevice(c->device));
    drain_profile(c);
    if (out) *out = c->prof;
    if (reset) c->prof = coala_comm_profile_t{};
    if (enable >= 0) c->profile = enable != 0;
    return COALA_OK;
}

int coala_cache_fetch_distributed(coala_cache_t* h, coala_comm_t* c, float* out, const int64_t* idx, int64_t n, void* stream) {
    FetchCall f{h, c, out, idx, n, (hipStream_t)stream};
    return fetch(f);
}

int coala_cache_fetch_distributed_bucketed(coala_cache_t* h, coala_comm_t* c, float* out, const int64_t* idx, int64_t n,
                                           const int64_t* counts_dev, void* stream) {
    if (!counts_dev) return fail(COALA_EINVAL, "null bucket counts");
    FetchCall f{h, c, out, idx, n, (hipStream_t)stream};
    f.bucket_counts_dev = counts_dev;
    return fetch(f);
}

int coala_comm_counts_begin(coala_comm_t* c, const int64_t* counts_dev, void* stream, int64_t* ticket_out) {
    if (!c || !counts_dev || !ticket_out) return fail(COALA_EINVAL, "null argument");
    if (int rc = refuse_abandoned(c)) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t G = (size_t)c->nranks;
    const CountsSlot slot = counts_slot(c, c->ahead_calls);
    if (c->ahead_calls >= coala_comm::kCountsRing) HIPCHK(hipEventSynchronize(slot.ev)); // the slot's previous exchange has landed
    // the peers are about to enter the collective: from here on a rank that fails abandons the communicator, as in fetch.  (Behind the
    // collective too: a local failure must not leave this rank's ticket counter behind its peers'.)
    if (hipMemcpyAsync(slot.dev, counts_dev, G * sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return abandon(c, fail(COALA_EHIP, "count exchange issued ahead: staging the counts failed: %s", hipGetErrorString(hipGetLastError())));
    if (int rc = c->tr->all_to_all_i64(slot.dev, slot.dev + G, st)) return abandon(c, rc);
    if (hipMemcpyAsync(slot.host, slot.dev, 2 * G * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipEventRecord(slot.ev, st) != hipSuccess)
        return abandon(c, fail(COALA_EHIP, "count exchange issued ahead: reading the counts back failed: %s", hipGetErrorString(hipGetLastError())));
    *ticket_out = (int64_t)c->ahead_calls++;
    return COALA_OK;
}

int coala_cache_fetch_distributed_bucketed_ahead(coala_cache_t* h, coala_comm_t* c, float* out, const int64_t* idx, int64_t n, int64_t ticket,
                                                 void* stream) {
    if (!c) return fail(COALA_EINVAL, "null handle");
    if (ticket < 0 || (uint64_t)ticket >= c->ahead_calls || c->ahead_calls - (uint64_t)ticket > (uint64_t)coala_comm::kCountsRing)
        return fail(COALA_EINVAL, "ticket %lld is not one of the last %d count exchanges", (long long)ticket, coala_comm::kCountsRing);
    HIPCHK(hipSetDevice(c->device));
    const CountsSlot slot = counts_slot(c, (uint64_t)ticket);
    HIPCHK(hipEventSynchronize(slot.ev)); // issued a step or two ago: normally complete long since
    FetchCall f{h, c, out, idx, n, (hipStream_t)stream};
    f.bucket_counts_dev = slot.dev, f.counts_host = slot.host;
    return fetch(f);
}

} // extern "C"
