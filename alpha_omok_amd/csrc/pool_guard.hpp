// pool_guard.hpp -- the pure part of the guarded allocation mode (AO_POOL_GUARD / AO_POOL_FILL, host_handle.hpp): the layout of a
// guarded block, the comparison of a guard's image with the fill byte, the text of a damage report and the process-wide list of
// the guarded blocks that are alive. No HIP call here: tests/host/pool_guard_main.cpp drives it on plain host memory.
//
//     base                      ptr = base + guard            ptr + bytes            ptr + bytes + guard
//      | front guard (guard B)   | body (bytes B, what the owner asked for) | rear guard (guard B) |
//
// All three parts are written with the fill byte before the owner sees the block. Nothing but the owner's kernels and copies
// writes to it afterwards, so a guard byte that differs from the fill is a stray write.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace ao {
namespace guard {

constexpr size_t kGuardAlign = 4096;   // keeps ptr as aligned as hipMalloc's base for the kernels' 16-byte accesses
constexpr int kReportMax = 8;          // damaged blocks described in one report; the rest are counted

// AO_POOL_GUARD's value -> guard bytes: 0 (mode off) for nothing, zero, negative or not a number, else rounded up to 4096
inline size_t guard_bytes(const char* text) {
    if (!text || !*text) return 0;
    char* end = nullptr;
    const long long v = std::strtoll(text, &end, 10);
    if (end == text || v <= 0) return 0;
    return (static_cast<size_t>(v) + kGuardAlign - 1) / kGuardAlign * kGuardAlign;
}

// AO_POOL_FILL's value -> the fill byte: 0..255, and 255 for nothing or anything else
inline uint8_t fill_byte(const char* text) {
    if (!text || !*text) return 255;
    char* end = nullptr;
    const long v = std::strtol(text, &end, 0);
    if (end == text || v < 0 || v > 255) return 255;
    return static_cast<uint8_t>(v);
}

inline size_t total_bytes(size_t bytes, size_t guard) { return guard + bytes + guard; }
inline size_t body_offset(size_t guard) { return guard; }
inline size_t rear_offset(size_t bytes, size_t guard) { return guard + bytes; }

// the bytes of one guard that differ from the fill: how many, the index of the first (lowest address) and its value
struct Scan {
    int64_t count = 0;
    int64_t first = -1;
    uint8_t value = 0;
};

inline Scan scan(const uint8_t* image, size_t n, uint8_t fill) {
    Scan s;
    for (size_t i = 0; i < n; ++i) {
        if (image[i] == fill) continue;
        if (s.count == 0) {
            s.first = static_cast<int64_t>(i);
            s.value = image[i];
        }
        ++s.count;
    }
    return s;
}

// one guarded block that is alive
struct Entry {
    int device = 0;
    void* ptr = nullptr;   // what the owner got: base + guard
    size_t bytes = 0;      // what the owner asked for
    size_t guard = 0;
    uint8_t fill = 255;
    uint64_t ordinal = 0;  // counts the guarded allocations of the process: leads to the allocation site
};

// what a check found in the two guards of one block
struct Damage {
    Scan front, rear;
    bool any() const { return front.count + rear.count > 0; }
    int64_t count() const { return front.count + rear.count; }
};

inline Damage compare(const uint8_t* front_image, const uint8_t* rear_image, size_t guard, uint8_t fill) {
    Damage d;
    d.front = scan(front_image, guard, fill);
    d.rear = scan(rear_image, guard, fill);
    return d;
}

// "block #7 (900 B, device 0): 3 damaged bytes, first at start-1, found 0x00 (fill 0xff)": the first damaged byte is the one at
// the lowest address; start-k is k bytes before the body's first byte (k = 1 .. guard), end+k is k bytes after its last byte's
// successor (k = 0 .. guard-1, end+0 being the first byte after the block).
inline std::string describe(const Entry& e, const Damage& d) {
    const bool in_front = d.front.count > 0;
    const Scan& s = in_front ? d.front : d.rear;
    const long long off = in_front ? static_cast<long long>(e.guard) - s.first : static_cast<long long>(s.first);
    char buf[224];
    std::snprintf(buf, sizeof buf, "block #%llu (%llu B, device %d): %lld damaged byte%s, first at %s%lld, found 0x%02x (fill 0x%02x)",
                  static_cast<unsigned long long>(e.ordinal), static_cast<unsigned long long>(e.bytes), e.device,
                  static_cast<long long>(d.count()), d.count() == 1 ? "" : "s", in_front ? "start-" : "end+", off,
                  static_cast<unsigned>(s.value), static_cast<unsigned>(e.fill));
    return buf;
}

// The report of one check: the first kReportMax descriptions, one per line, then how many more there are; cut to cap - 1
// characters and always terminated (cap <= 0 or no msg: nothing is written).
inline void write_report(const std::vector<std::string>& lines, char* msg, int cap) {
    if (!msg || cap <= 0) return;
    std::string all;
    const size_t shown = lines.size() < static_cast<size_t>(kReportMax) ? lines.size() : static_cast<size_t>(kReportMax);
    for (size_t i = 0; i < shown; ++i) {
        if (i) all += '\n';
        all += lines[i];
    }
    if (lines.size() > shown) all += "\n... and " + std::to_string(lines.size() - shown) + " more";
    const size_t n = all.size() < static_cast<size_t>(cap - 1) ? all.size() : static_cast<size_t>(cap - 1);
    std::memcpy(msg, all.data(), n);
    msg[n] = '\0';
}

// The guarded blocks of the process that are alive, in allocation order, and the damage found when a block was freed (sticky:
// kept until a check reports it). train_async creates handles on a worker thread: every access holds the mutex.
struct Registry {
    std::mutex mu;
    std::vector<Entry> live;
    std::vector<std::string> sticky;
    uint64_t next_ordinal = 0;

    // the caller holds mu for these
    Entry& add(int device, void* ptr, size_t bytes, size_t guard_b, uint8_t fill) {
        Entry e;
        e.device = device; e.ptr = ptr; e.bytes = bytes; e.guard = guard_b; e.fill = fill; e.ordinal = next_ordinal++;
        live.push_back(e);
        return live.back();
    }
    int find(const void* ptr) const {
        for (size_t i = 0; i < live.size(); ++i)
            if (live[i].ptr == ptr) return static_cast<int>(i);
        return -1;
    }
    void remove(int index) { live.erase(live.begin() + index); }
    // ends a check: the sticky reports first, then `fresh`; the sticky ones are forgotten
    std::vector<std::string> take_report(const std::vector<std::string>& fresh) {
        std::vector<std::string> all;
        all.swap(sticky);
        all.insert(all.end(), fresh.begin(), fresh.end());
        return all;
    }
};

// one object per process, whichever translation unit asks
inline Registry& registry() {
    static Registry r;
    return r;
}

}  // namespace guard
}  // namespace ao
