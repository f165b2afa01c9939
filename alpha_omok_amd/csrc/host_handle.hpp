// host_handle.hpp -- the host plumbing every handle of the C ABI shares (ao_engine, ao_net, ao_replay, ao_rollout, ao_ttt,
// ao_positions): error string and HIP check, the create shape, device allocations that are freed in one place, grow-only
// device buffers, the dispatch on a board's 64-cell words, and the HIP-event timing ring. Host code only: no kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "pool_guard.hpp"

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
//
// Guarded mode (pool_guard.hpp), read from the environment at every allocation: AO_POOL_GUARD=<bytes> (rounded up to 4096) puts
// that many guard bytes in front of and behind the block, and AO_POOL_FILL=<0..255> (default 255) is written to both guards and to
// the whole body before the owner sees the block. With AO_POOL_GUARD unset or 0 the allocation is the plain hipMalloc it always
// was. The mode costs allocation-time (and free-time) work only: no kernel and no launch knows about it.
struct DevPool {
    std::vector<void*> blocks;

    // the one hipMalloc of the library: `bytes` of device memory for this owner, freed by release() or free_all()
    hipError_t alloc_bytes(void** out, size_t bytes) {
        *out = nullptr;
        const size_t g = guard::guard_bytes(std::getenv("AO_POOL_GUARD"));
        void* p = nullptr;
        if (g == 0) {
            const hipError_t st = hipMalloc(&p, std::max<size_t>(bytes, 16));
            if (st != hipSuccess) return st;
        } else {
            const uint8_t fill = guard::fill_byte(std::getenv("AO_POOL_FILL"));
            const size_t total = guard::total_bytes(bytes, g);
            void* base = nullptr;
            int dev = 0;
            hipError_t st = hipGetDevice(&dev);
            if (st == hipSuccess) st = hipMalloc(&base, total);
            if (st != hipSuccess) return st;
            // complete before any stream of the owner can touch the block
            st = hipMemset(base, fill, total);
            if (st == hipSuccess) st = hipDeviceSynchronize();
            if (st != hipSuccess) {
                (void)hipFree(base);
                return st;
            }
            p = static_cast<unsigned char*>(base) + guard::body_offset(g);
            guard::Registry& reg = guard::registry();
            std::lock_guard<std::mutex> lock(reg.mu);
            reg.add(dev, p, bytes, g, fill);
        }
        blocks.push_back(p);
        *out = p;
        return hipSuccess;
    }
    template <class T>
    int alloc(HandleBase* h, T** out, size_t count) {
        void* p = nullptr;
        const hipError_t st = alloc_bytes(&p, count * sizeof(T));
        if (st != hipSuccess) return h->fail(std::string("hipMalloc(") + std::to_string(count * sizeof(T)) + " B): " + hipGetErrorString(st));
        *out = static_cast<T*>(p);
        return 0;
    }
    void release(void* p) {                        // frees one block now
        const auto it = std::find(blocks.begin(), blocks.end(), p);
        if (it == blocks.end()) return;
        free_block(p);
        blocks.erase(it);
    }
    void free_all() {
        for (void* p : blocks) free_block(p);
        blocks.clear();
    }

private:
    // a guarded block's guards are read once more before it goes: damage found here waits for the next ao_guard_check
    static void free_block(void* p) {
        guard::Registry& reg = guard::registry();
        std::lock_guard<std::mutex> lock(reg.mu);
        const int i = reg.find(p);
        if (i < 0) {
            (void)hipFree(p);
            return;
        }
        const guard::Entry e = reg.live[i];
        reg.remove(i);
        guard::Damage d;
        if (read_guards(e, &d) == hipSuccess && d.any()) reg.sticky.push_back(guard::describe(e, d) + " [found when freed]");
        (void)hipFree(static_cast<unsigned char*>(p) - guard::body_offset(e.guard));
    }

public:
    // waits for the current device (the block's) and compares both guards of `e` with its fill byte
    static hipError_t read_guards(const guard::Entry& e, guard::Damage* d) {
        std::vector<uint8_t> img(2 * e.guard);
        const unsigned char* body = static_cast<const unsigned char*>(e.ptr);
        hipError_t st = hipDeviceSynchronize();
        if (st == hipSuccess) st = hipMemcpy(img.data(), body - e.guard, e.guard, hipMemcpyDeviceToHost);
        if (st == hipSuccess) st = hipMemcpy(img.data() + e.guard, body + e.bytes, e.guard, hipMemcpyDeviceToHost);
        if (st != hipSuccess) return st;
        *d = guard::compare(img.data(), img.data() + e.guard, e.guard, e.fill);
        return hipSuccess;
    }
};

// ao_guard_check: every device that has guarded blocks is waited for, all guards are read back, and the damaged blocks -- those
// found at free time since the last check first -- are described in msg. A damaged guard is written with its fill again, so the
// next check reports only what happened after this one. The current device is the same afterwards.
inline int guard_check(int32_t* blocks, int32_t* damaged, char* msg, int cap) {
    guard::Registry& reg = guard::registry();
    std::lock_guard<std::mutex> lock(reg.mu);
    if (blocks) *blocks = static_cast<int32_t>(reg.live.size());
    if (damaged) *damaged = 0;
    if (msg && cap > 0) msg[0] = '\0';
    int dev0 = 0;
    hipError_t st = reg.live.empty() ? hipSuccess : hipGetDevice(&dev0);
    std::vector<std::string> fresh;
    int cur = dev0;
    for (const guard::Entry& e : reg.live) {
        if (st != hipSuccess) break;
        if (e.device != cur) {
            st = hipSetDevice(e.device);
            if (st != hipSuccess) break;
            cur = e.device;
        }
        guard::Damage d;
        st = DevPool::read_guards(e, &d);
        if (st != hipSuccess || !d.any()) continue;
        fresh.push_back(guard::describe(e, d));
        unsigned char* body = static_cast<unsigned char*>(e.ptr);
        if (d.front.count) st = hipMemset(body - e.guard, e.fill, e.guard);
        if (st == hipSuccess && d.rear.count) st = hipMemset(body + e.bytes, e.fill, e.guard);
        if (st == hipSuccess) st = hipDeviceSynchronize();
    }
    if (cur != dev0) (void)hipSetDevice(dev0);
    if (st != hipSuccess) {
        guard::write_report({std::string("ao_guard_check: ") + hipGetErrorString(st)}, msg, cap);
        return 1;
    }
    const std::vector<std::string> all = reg.take_report(fresh);
    if (damaged) *damaged = static_cast<int32_t>(all.size());
    guard::write_report(all, msg, cap);
    return 0;
}

// ao_guard_block: the index-th live guarded block, in allocation order; 1 past the end
inline int guard_block(int32_t index, void** ptr, int64_t* bytes, int64_t* guard_b) {
    guard::Registry& reg = guard::registry();
    std::lock_guard<std::mutex> lock(reg.mu);
    if (index < 0 || static_cast<size_t>(index) >= reg.live.size()) return 1;
    const guard::Entry& e = reg.live[index];
    if (ptr) *ptr = e.ptr;
    if (bytes) *bytes = static_cast<int64_t>(e.bytes);
    if (guard_b) *guard_b = static_cast<int64_t>(e.guard);
    return 0;
}

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
