// host_handle.hpp -- the host plumbing every handle of the C ABI shares (ao_engine, ao_net, ao_replay, ao_rollout, ao_ttt,
// ao_positions): error string and HIP check, the create shape, device allocations that are freed in one place, grow-only
// device buffers, the dispatch on a board's 64-cell words, and the HIP-event timing ring. Host code only: no kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

// `h` is a handle (a HandleBase): a failed HIP call becomes its error message and the caller returns 1
#define AO_HIP(h, call)                                                                       \
    do {                                                                                      \
        hipError_t st_ = (call);                                                              \
        if (st_ != hipSuccess)                                                                \
            return (h)->fail(std::string(#call) + ": " + hipGetErrorString(st_));             \
    } while (0)

namespace ao {

struct HandleBase {
    std::string err;   // what ao_*_last_error(handle) returns
    int fail(const std::string& m) { err = m; return 1; }
};

// what ao_*_last_error(NULL) returns for handle type H: the failed create (or snapshot check) of this thread. One object per
// thread and type, whichever translation unit asks.
template <class H>
inline std::string& create_error() {
    static thread_local std::string s;
    return s;
}

// The end of every ao_*_create: `h` is a new handle, `failed` what its create_impl returned. On failure the message goes to the
// thread's create-error string and the handle's own destroy releases whatever exists (it copes with a half-built handle).
template <class H>
int finish_create(H* h, int failed, H** out, void (*destroy)(H*), const char* prefix = "") {
    *out = failed ? nullptr : h;
    if (!failed) return 0;
    create_error<H>() = prefix + h->err;
    destroy(h);
    return 1;
}

// Device allocations of one owner, freed together by free_all() -- from the handle's destroy, after the device is set and its
// work is done. No destructor frees: the handles are plain structs deleted by ao_*_destroy.
struct DevPool {
    std::vector<void*> blocks;

    template <class T>
    int alloc(HandleBase* h, T** out, size_t count) {
        void* p = nullptr;
        const hipError_t st = hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16));
        if (st != hipSuccess) return h->fail(std::string("hipMalloc(") + std::to_string(count * sizeof(T)) + " B): " + hipGetErrorString(st));
        blocks.push_back(p);
        *out = static_cast<T*>(p);
        return 0;
    }
    void adopt(void* p) { blocks.push_back(p); }   // a block from a hipMalloc of the owner's own: freed with the rest
    void release(void* p) {                        // frees one block now
        const auto it = std::find(blocks.begin(), blocks.end(), p);
        if (it == blocks.end()) return;
        (void)hipFree(p);
        blocks.erase(it);
    }
    void free_all() {
        for (void* p : blocks) (void)hipFree(p);
        blocks.clear();
    }
};

// A grow-only device buffer inside its owner's pool. reserve(h, n): at least n elements afterwards -- the old contents are not
// kept, and nothing queued may still use them (the caller synchronises before it grows). After a failed allocation p is null
// and n is 0. For a fixed n this is "allocate on first use".
template <class T>
struct DevBuf {
    DevPool* pool;
    T* p = nullptr;
    size_t n = 0;
    explicit DevBuf(DevPool* owner) : pool(owner) {}

    int reserve(HandleBase* h, size_t count) {
        if (p && count <= n) return 0;
        pool->release(p);
        p = nullptr;
        n = 0;
        if (pool->alloc(h, &p, count)) return 1;
        n = count;
        return 0;
    }
};

// HIP-event timing of launches on a stream: a ring of event pairs; when it is full the older half is waited for and summed up.
struct EventTimer {
    const int ring;
    std::vector<hipEvent_t> ev0, ev1;
    int ring_head = 0, ring_count = 0;
    bool on = false;
    int stride = 1;          // every stride-th tick is timed
    unsigned ticks = 0;
    double ms_total = 0.0;
    int64_t launches = 0;
    explicit EventTimer(int ring_size) : ring(ring_size) {}

    // ao_tree_timing / ao_net_conv_timing: reads and resets the totals, then times every tick (enable 1), every enable-th
    // (enable > 1) or none (0). The events are created by the first call that enables.
    int enable(HandleBase* h, int enable, double* ms, int64_t* count) {
        if (ev0.empty() && enable) {
            ev0.resize(ring);
            ev1.resize(ring);
            for (int i = 0; i < ring; ++i) {
                AO_HIP(h, hipEventCreate(&ev0[i]));
                AO_HIP(h, hipEventCreate(&ev1[i]));
            }
        }
        read_and_reset(ms, count);
        on = enable != 0;
        stride = enable > 1 ? enable : 1;
        ticks = 0;
        return 0;
    }
    bool tick() { return on && (ticks++ % static_cast<unsigned>(stride) == 0u); }   // is this launch (or forward) timed?
    void begin(hipStream_t s) {
        if (ring_count == ring) harvest(ring / 2);
        (void)hipEventRecord(ev0[ring_head], s);
    }
    void end(hipStream_t s) {
        (void)hipEventRecord(ev1[ring_head], s);
        ring_head = (ring_head + 1) % ring;
        ++ring_count;
    }
    void harvest(int count) {   // the `count` oldest pairs
        for (int i = 0; i < count; ++i) {
            const int idx = (ring_head - ring_count + ring * 2) % ring;
            (void)hipEventSynchronize(ev1[idx]);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev0[idx], ev1[idx]) == hipSuccess) {
                ms_total += ms;
                launches += 1;
            }
            --ring_count;
        }
    }
    void read_and_reset(double* ms, int64_t* count) {
        harvest(ring_count);
        if (ms) *ms = ms_total;
        if (count) *count = launches;
        ms_total = 0.0;
        launches = 0;
    }
    void destroy() {
        for (auto ev : ev0) (void)hipEventDestroy(ev);
        for (auto ev : ev1) (void)hipEventDestroy(ev);
        ev0.clear();
        ev1.clear();
    }
};

// NCH = the 64-cell words of a board, (A + 63) / 64 in 1..4: a template argument of every tree, rollout, position, read-out and
// snapshot kernel. AO_DISPATCH_NCH(nch, statement using NCH) runs the statement with NCH as a constant.
inline int nch_of_cells(int A) { return (A + 63) / 64; }

}  // namespace ao

#define AO_DISPATCH_NCH(nch, ...)                                  \
    switch (nch) {                                                 \
        case 1: { constexpr int NCH = 1; __VA_ARGS__; } break;     \
        case 2: { constexpr int NCH = 2; __VA_ARGS__; } break;     \
        case 3: { constexpr int NCH = 3; __VA_ARGS__; } break;     \
        default: { constexpr int NCH = 4; __VA_ARGS__; } break;    \
    }
