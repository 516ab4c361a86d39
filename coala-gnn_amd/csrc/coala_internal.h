// coala_internal.h -- shared by the translation units of libcoala_hip.so (not part of the ABI).
#ifndef COALA_INTERNAL_H
#define COALA_INTERNAL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

// Records a thread-local message for coala_last_error() and returns `code`.
int coala_fail_(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define COALA_HIPCHK(expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return coala_fail_(COALA_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                               __LINE__);                                                                    \
    } while (0)

// Launch geometry of the sampler (coala_sampler.hip) and of the block ops (coala_block_ops.hip).
constexpr int kBlock = 256; // threads per block
constexpr int kWavesPerBlock = kBlock / 64;

// blocks for n items at `block` items per block: at least one, at most `cap` (the cache's kernels: chunks or tiles at one per wave)
inline int grid1d(int64_t n, int block, int cap) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// log2 of a power of two, -1 for every other value
inline int ilog2_exact(uint64_t v) {
    if (v == 0 || (v & (v - 1))) return -1;
    int s = 0;
    while ((1ull << s) != v) ++s;
    return s;
}

// Device scratch *p of *cap elements that has to hold `need`: kept when it is large enough, else -- after everything enqueued on `st`, which
// may still use it, has finished -- replaced by one of the capacity doubled (from `first`) until it fits.  The contents are not kept.  A
// failure leaves *cap 0, so the next call tries again.
inline int grow(void** p, uint64_t* cap, uint64_t need, size_t elem, hipStream_t st, uint64_t first = 1024) {
    if (need <= *cap) return COALA_OK;
    COALA_HIPCHK(hipStreamSynchronize(st));
    uint64_t c = *cap ? *cap : first;
    while (c < need) c *= 2;
    *cap = 0;
    if (*p) COALA_HIPCHK(hipFree(*p));
    *p = nullptr;
    COALA_HIPCHK(hipMalloc(p, c * elem));
    *cap = c;
    return COALA_OK;
}

// What a handle (cache, communicator) owns on the device is ordered by the stream its calls are enqueued on.  A caller that moves to another
// stream keeps that order: the new stream first waits (no host wait) for what the handle enqueued last on the old one.
struct StreamOrder {
    hipStream_t stream = nullptr;
    bool set = false;
    hipEvent_t ev = nullptr; // created on the first move
    ~StreamOrder() { if (ev) (void)hipEventDestroy(ev); }
    int follow(hipStream_t s) {
        if (set && stream != s) {
            if (!ev) COALA_HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            // (a stream the caller has destroyed in the meantime has nothing left to wait for)
            if (hipEventRecord(ev, stream) == hipSuccess) COALA_HIPCHK(hipStreamWaitEvent(s, ev, 0));
            else (void)hipGetLastError();
        }
        stream = s, set = true;
        return COALA_OK;
    }
};

// Timing events of a profiling handle, reused: take() hands out a free one or creates one (nullptr when that fails), give() returns it.
struct EventPool {
    std::vector<hipEvent_t> idle;
    ~EventPool() { for (hipEvent_t e : idle) (void)hipEventDestroy(e); }
    hipEvent_t take() {
        hipEvent_t e = idle.empty() ? nullptr : idle.back();
        if (e) idle.pop_back();
        else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        return e;
    }
    void give(hipEvent_t e) { idle.push_back(e); }
};

// The split-phase serve calls with an event ON a launch instead of behind it (coala_cache.hip; used by the distributed fetch, coala_comm.cpp):
// begin_ev rides on the probe's launch, end_ev on the last fill launch of the call.  *rode = the event that really rides there: the caller's, or
// the handle's own profiling event of that launch (a profiling handle keeps the dispatches' event slots: fine to wait on, not to time with), or
// NULL when the call launched nothing (the caller then records its event the plain way).
struct coala_cache;
struct coala_row_redirect;
extern "C" {
int coala_serve_probe_redirect_ev_(coala_cache* h, float* out, const int64_t* ids, int64_t n, const coala_row_redirect* redirect, void* stream,
                                   hipEvent_t begin_ev, hipEvent_t* rode);
int coala_serve_fill_ranges_ev_(coala_cache* h, float* out, const int64_t* ids, int64_t n, const int64_t* begins, const int64_t* ends, int n_ranges,
                                void* stream, hipEvent_t end_ev, hipEvent_t* rode);
}
#endif
