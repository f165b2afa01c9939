// replay_snapshot.hip -- the replay memory out of HBM and back in: k_replay_pack writes deque entries as the packed arrays of
// ao_replay_snapshot (include/omok_hip.h), k_replay_unpack writes ring slots from them, k_replay_count sizes the
// variable-length parts first.
//
// Reference (paths relative to /root/reference/2_AlphaOmok/): main.save_dataset pickles the deque (main.py:345-348) and
// main.load_data rebuilds the deque from the pickle (main.py:351-365). Here the planes (0/1) become one bit per cell and pi
// (float64, sparse) a cell mask and its non-zero values, on the device, and only packed bytes cross the bus.
//
// One wavefront per entry, 64 lanes over 64 cells per step: __ballot of "value is 1.0f" IS the plane word, __ballot of "pi
// pattern is not zero" IS the mask word, a lane's rank among the set bits below it plus the popcounts of the earlier words is
// its place in pi_val. What steers control flow (entry, plane, word) is wave-uniform; cells at or above A never vote. Values
// move as bit patterns (uint32 / uint64), so -0.0, NaN payloads and subnormals come through untouched. All element offsets
// are 64-bit: the ring exceeds 2^31 bytes at production size. Byte movers: no LDS, HBM-bound.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "replay_ring.hpp"
#include "replay_snapshot_check.hpp"

namespace ao {

constexpr uint32_t kOneF32 = 0x3f800000u;     // the pattern of 1.0f
constexpr uint32_t kNoRaw = 0xffffffffu;      // raw index of a kind-0 entry
constexpr int kRsBlock = 256;                 // four wavefronts, four entries per workgroup and step
constexpr int64_t kRsMaxGrid = 4096;          // bounded grid, entries taken in grid stride

struct RsRing {                               // the three rings as bit patterns
    uint32_t* s; uint64_t* pi; uint32_t* z;
    int64_t cap;
    int C, A, W;
};

struct RsChunk {                              // a chunk of packed entries in the device workspace
    uint8_t* kind; uint32_t* z; uint64_t* bits; uint64_t* mask; uint64_t* pival; uint32_t* raw;
    const uint32_t* pioff;                    // [len] first pi_val of the entry, inside the chunk
    const uint32_t* rawidx;                   // [len] its index in raw, inside the chunk; kNoRaw for kind 0
    int64_t len, npi, nraw;                   // entries, pi values, raw entries of the chunk: every store and load is bounded by them
};

__device__ __forceinline__ int rs_lane() { return static_cast<int>(threadIdx.x) & 63; }
__device__ __forceinline__ int64_t rs_wave() { return (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) >> 6; }
__device__ __forceinline__ int64_t rs_waves() { return (gridDim.x * static_cast<int64_t>(blockDim.x)) >> 6; }

// entries slot0 .. of the ring (wrapping) -> nnz[i] = non-zero pi patterns, kind[i] = 1 when a plane value is neither +0.0f nor 1.0f
__global__ __launch_bounds__(kRsBlock) void k_replay_count(RsRing g, int64_t slot0, int64_t n, int32_t* __restrict__ nnz,
                                                           uint8_t* __restrict__ kind) {
    const int lane = rs_lane();
    for (int64_t i = rs_wave(); i < n; i += rs_waves()) {          // (wave-uniform)
        const int64_t slot = (slot0 + i) % g.cap;
        const uint32_t* sp = g.s + slot * g.C * g.A;
        uint64_t other = 0;
        for (int c = 0; c < g.C; ++c)
            for (int w = 0; w < g.W; ++w) {
                const int cell = 64 * w + lane;
                const bool valid = cell < g.A;
                const uint32_t u = valid ? sp[static_cast<int64_t>(c) * g.A + cell] : 0u;
                other |= __ballot(valid && u != 0u && u != kOneF32);
            }
        const uint64_t* pp = g.pi + slot * g.A;
        int cnt = 0;
        for (int w = 0; w < g.W; ++w) {
            const int cell = 64 * w + lane;
            const bool valid = cell < g.A;
            const uint64_t p = valid ? pp[cell] : 0ull;
            cnt += __popcll(__ballot(valid && p != 0ull));
        }
        if (lane == 0) {
            nnz[i] = cnt;
            kind[i] = other ? 1 : 0;
        }
    }
}

// entries slot0 .. of the ring (wrapping) -> chunk entries 0 .. len; pioff / rawidx come from the count pass
__global__ __launch_bounds__(kRsBlock) void k_replay_pack(RsRing g, RsChunk d, int64_t slot0) {
    const int lane = rs_lane();
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t i = rs_wave(); i < d.len; i += rs_waves()) {      // (wave-uniform)
        const int64_t slot = (slot0 + i) % g.cap;
        const uint32_t ridx = d.rawidx[i];
        const bool israw = ridx != kNoRaw;
        const uint32_t* sp = g.s + slot * g.C * g.A;
        for (int c = 0; c < g.C; ++c)
            for (int w = 0; w < g.W; ++w) {
                const int cell = 64 * w + lane;
                const bool valid = cell < g.A;
                const uint32_t u = valid ? sp[static_cast<int64_t>(c) * g.A + cell] : 0u;
                const uint64_t m = __ballot(valid && u == kOneF32);
                if (lane == 0) d.bits[(i * g.C + c) * g.W + w] = israw ? 0ull : m;
                if (israw && valid && ridx < d.nraw) d.raw[(static_cast<int64_t>(ridx) * g.C + c) * g.A + cell] = u;
            }
        const uint64_t* pp = g.pi + slot * g.A;
        int64_t base = d.pioff[i];
        for (int w = 0; w < g.W; ++w) {
            const int cell = 64 * w + lane;
            const bool valid = cell < g.A;
            const uint64_t p = valid ? pp[cell] : 0ull;
            const bool nz = valid && p != 0ull;
            const uint64_t m = __ballot(nz);
            if (lane == 0) d.mask[i * g.W + w] = m;
            const int64_t at = base + __popcll(m & below);
            if (nz && at < d.npi) d.pival[at] = p;
            base += __popcll(m);
        }
        if (lane == 0) {
            d.kind[i] = israw ? 1 : 0;
            d.z[i] = g.z[slot];
        }
    }
}

// chunk entries 0 .. len -> ring slots slot0 .. (wrapping; the host hands a launch at most cap entries, so no two waves share
// a slot). Every byte of a slot is written: zero cells of the planes and of pi are stores.
__global__ __launch_bounds__(kRsBlock) void k_replay_unpack(RsRing g, RsChunk d, int64_t slot0) {
    const int lane = rs_lane();
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t i = rs_wave(); i < d.len; i += rs_waves()) {      // (wave-uniform)
        const int64_t slot = (slot0 + i) % g.cap;
        const uint32_t ridx = d.rawidx[i];
        const bool israw = d.kind[i] != 0 && ridx < d.nraw;
        uint32_t* sp = g.s + slot * g.C * g.A;
        for (int c = 0; c < g.C; ++c)
            for (int w = 0; w < g.W; ++w) {
                const int cell = 64 * w + lane;
                if (cell >= g.A) continue;
                uint32_t u;
                if (israw) u = d.raw[(static_cast<int64_t>(ridx) * g.C + c) * g.A + cell];
                else u = ((d.bits[(i * g.C + c) * g.W + w] >> lane) & 1ull) ? kOneF32 : 0u;
                sp[static_cast<int64_t>(c) * g.A + cell] = u;
            }
        uint64_t* pp = g.pi + slot * g.A;
        int64_t base = d.pioff[i];
        for (int w = 0; w < g.W; ++w) {
            const int cell = 64 * w + lane;
            const uint64_t m = d.mask[i * g.W + w];
            const int64_t at = base + __popcll(m & below);
            if (cell < g.A) pp[cell] = (((m >> lane) & 1ull) && at < d.npi) ? d.pival[at] : 0ull;
            base += __popcll(m);
        }
        if (lane == 0) g.z[slot] = d.z[i];
    }
}

// ----------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------
struct RsWork {                               // device workspace of one call, freed when the call returns
    DevPool pool;
    unsigned char* buf = nullptr;             // a chunk's packed sections
    uint32_t* off = nullptr;                  // [2][m] pioff, rawidx
    int32_t* nnz = nullptr;                   // [m] count pass
    uint8_t* ckind = nullptr;                 // [m] count pass
    ~RsWork() { pool.free_all(); }
};

struct RsShape {
    int C, A, W;
    int64_t fixed, raw_bytes, entry_max, chunk_bytes, m;   // m: entries a chunk (and a count block) holds at most
};

constexpr int64_t kRsDefaultChunk = 64ll << 20, kRsMaxChunk = 1ll << 30;

static RsShape rs_shape(const ao_replay* r, int64_t chunk_bytes, int64_t n) {
    RsShape h;
    h.C = r->C; h.A = r->A; h.W = (r->A + 63) / 64;
    h.fixed = 5 + 8ll * h.W * (h.C + 1);
    h.raw_bytes = 4ll * h.C * h.A;
    h.entry_max = h.fixed + 8ll * h.A + h.raw_bytes;
    h.chunk_bytes = chunk_bytes == 0 ? kRsDefaultChunk : std::min(chunk_bytes, kRsMaxChunk);
    h.m = std::max<int64_t>(1, std::min(n, h.chunk_bytes / h.fixed + 1));
    return h;
}

static RsRing rs_ring(const ao_replay* r) {
    return RsRing{reinterpret_cast<uint32_t*>(r->s_ring), reinterpret_cast<uint64_t*>(r->pi_ring),
                  reinterpret_cast<uint32_t*>(r->z_ring), r->cap, r->C, r->A, (r->A + 63) / 64};
}

static inline size_t rs_align8(size_t x) { return (x + 7) & ~static_cast<size_t>(7); }

struct RsLayout { size_t kind, z, bits, mask, pival, raw, total; };

static RsLayout rs_layout(const RsShape& h, int64_t len, int64_t npi, int64_t nraw) {
    RsLayout l;
    l.kind = 0;
    l.z = rs_align8(static_cast<size_t>(len));
    l.bits = l.z + rs_align8(4 * static_cast<size_t>(len));
    l.mask = l.bits + 8 * static_cast<size_t>(len) * h.C * h.W;
    l.pival = l.mask + 8 * static_cast<size_t>(len) * h.W;
    l.raw = l.pival + 8 * static_cast<size_t>(npi);
    l.total = l.raw + static_cast<size_t>(nraw) * h.raw_bytes;
    return l;
}

static RsChunk rs_chunk(const RsWork& ws, const RsShape& h, const RsLayout& l, int64_t len, int64_t npi, int64_t nraw) {
    RsChunk d;
    d.kind = ws.buf + l.kind;
    d.z = reinterpret_cast<uint32_t*>(ws.buf + l.z);
    d.bits = reinterpret_cast<uint64_t*>(ws.buf + l.bits);
    d.mask = reinterpret_cast<uint64_t*>(ws.buf + l.mask);
    d.pival = reinterpret_cast<uint64_t*>(ws.buf + l.pival);
    d.raw = reinterpret_cast<uint32_t*>(ws.buf + l.raw);
    d.pioff = ws.off;
    d.rawidx = ws.off + h.m;
    d.len = len; d.npi = npi; d.nraw = nraw;
    return d;
}

static inline unsigned rs_grid(int64_t entries) {
    return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((entries + kRsBlock / 64 - 1) / (kRsBlock / 64), kRsMaxGrid)));
}

static int rs_alloc(ao_replay* r, RsWork& ws, const RsShape& h, bool chunks) {
    const size_t m = static_cast<size_t>(h.m);
    if (ws.pool.alloc(r, &ws.nnz, m) || ws.pool.alloc(r, &ws.ckind, m)) return 1;
    if (!chunks) return 0;
    // a chunk is closed by the entry that takes it to chunk_bytes, and holds at most m entries
    const int64_t bytes = std::min(h.chunk_bytes + h.entry_max, h.m * h.entry_max) + 64;
    return ws.pool.alloc(r, &ws.buf, static_cast<size_t>(bytes)) || ws.pool.alloc(r, &ws.off, 2 * m);
}

// count pass over deque entries [at, at + blk), blk <= h.m: per-entry nnz and kind on the host
static int rs_count(ao_replay* r, const RsWork& ws, int64_t at, int64_t blk, hipStream_t s, int32_t* nnz, uint8_t* kind) {
    hipLaunchKernelGGL(k_replay_count, dim3(rs_grid(blk)), dim3(kRsBlock), 0, s, rs_ring(r), (r->head + at) % r->cap, blk, ws.nnz,
                       ws.ckind);
    AO_HIP(r, hipGetLastError());
    AO_HIP(r, hipMemcpyAsync(nnz, ws.nnz, static_cast<size_t>(blk) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    AO_HIP(r, hipMemcpyAsync(kind, ws.ckind, static_cast<size_t>(blk), hipMemcpyDeviceToHost, s));
    AO_HIP(r, hipStreamSynchronize(s));
    return 0;
}

static int rs_totals(ao_replay* r, const RsWork& ws, const RsShape& h, int64_t first, int64_t n, hipStream_t s, int64_t* pv,
                     int64_t* re) {
    std::vector<int32_t> nnz(static_cast<size_t>(h.m));
    std::vector<uint8_t> kind(static_cast<size_t>(h.m));
    *pv = 0; *re = 0;
    for (int64_t done = 0; done < n; done += h.m) {
        const int64_t blk = std::min(h.m, n - done);
        if (rs_count(r, ws, first + done, blk, s, nnz.data(), kind.data())) return 1;
        for (int64_t k = 0; k < blk; ++k) { *pv += nnz[static_cast<size_t>(k)]; *re += kind[static_cast<size_t>(k)]; }
    }
    return 0;
}

}  // namespace ao

extern "C" {

int ao_replay_snapshot_check(const ao_replay_snapshot* snap) {
    const std::string why = ao::replay_snapshot_check(snap);
    if (why.empty()) return 0;
    ao::create_error<ao_replay>() = "ao_replay_snapshot_check: " + why;
    return 1;
}

int ao_replay_export_size(ao_replay* r, int64_t first, int64_t n, int64_t* pi_values, int64_t* raw_entries) {
    if (first < 0 || n < 0 || first + n > r->count) return r->fail("ao_replay_export_size: range outside the memory");
    int64_t pv = 0, re = 0;
    if (n > 0) {
        AO_HIP(r, hipSetDevice(r->device));
        AO_HIP(r, hipDeviceSynchronize());
        const ao::RsShape h = ao::rs_shape(r, 0, n);
        ao::RsWork ws;
        if (ao::rs_alloc(r, ws, h, false)) return 1;
        if (ao::rs_totals(r, ws, h, first, n, nullptr, &pv, &re)) return 1;
    }
    if (pi_values) *pi_values = pv;
    if (raw_entries) *raw_entries = re;
    return 0;
}

int ao_replay_export(ao_replay* r, int64_t first, int64_t n, ao_replay_snapshot* snap, int64_t chunk_bytes, void* stream) {
    using namespace ao;
    if (!snap) return r->fail("ao_replay_export: null snapshot");
    if (first < 0 || n < 0 || first + n > r->count) return r->fail("ao_replay_export: range outside the memory");
    if (chunk_bytes < 0) return r->fail("ao_replay_export: negative chunk_bytes");
    if (snap->entries < n) return r->fail("ao_replay_export: entries: the arrays hold " + std::to_string(snap->entries) + ", the range has " + std::to_string(n));
    if (n > 0 && (!snap->kind || !snap->z || !snap->bits || !snap->pi_mask)) return r->fail("ao_replay_export: kind / z / bits / pi_mask: null array");
    const RsShape h = rs_shape(r, chunk_bytes, n);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t pv = 0, re = 0;
    RsWork ws;
    if (n > 0) {
        AO_HIP(r, hipSetDevice(r->device));
        AO_HIP(r, hipDeviceSynchronize());
        if (rs_alloc(r, ws, h, true)) return 1;
        if (rs_totals(r, ws, h, first, n, s, &pv, &re)) return 1;
    }
    if (snap->pi_values < pv) return r->fail("ao_replay_export: pi_values: pi_val holds " + std::to_string(snap->pi_values) + ", the range needs " + std::to_string(pv));
    if (snap->raw_entries < re) return r->fail("ao_replay_export: raw_entries: raw holds " + std::to_string(snap->raw_entries) + ", the range needs " + std::to_string(re));
    if ((pv > 0 && !snap->pi_val) || (re > 0 && !snap->raw)) return r->fail("ao_replay_export: pi_val / raw: null array");

    std::vector<int32_t> nnz(static_cast<size_t>(h.m));
    std::vector<uint8_t> kind(static_cast<size_t>(h.m));
    std::vector<uint32_t> off(2 * static_cast<size_t>(h.m));
    int64_t pi_at = 0, raw_at = 0;                        // what the chunks before this one put into pi_val / raw
    for (int64_t done = 0; done < n;) {
        const int64_t blk = std::min(h.m, n - done);
        if (rs_count(r, ws, first + done, blk, s, nnz.data(), kind.data())) return 1;
        for (int64_t j = 0; j < blk;) {
            int64_t len = 0, bytes = 0, npi = 0, nraw = 0;
            while (j + len < blk && bytes < h.chunk_bytes) {
                const size_t k = static_cast<size_t>(j + len);
                off[static_cast<size_t>(len)] = static_cast<uint32_t>(npi);
                off[static_cast<size_t>(h.m + len)] = kind[k] ? static_cast<uint32_t>(nraw) : kNoRaw;
                bytes += h.fixed + 8ll * nnz[k] + (kind[k] ? h.raw_bytes : 0);
                npi += nnz[k];
                nraw += kind[k];
                ++len;
            }
            if (pi_at + npi > pv || raw_at + nraw > re) return r->fail("ao_replay_export: the memory changed during the export");
            const RsLayout l = rs_layout(h, len, npi, nraw);
            const RsChunk d = rs_chunk(ws, h, l, len, npi, nraw);
            AO_HIP(r, hipMemcpyAsync(ws.off, off.data(), static_cast<size_t>(len) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            AO_HIP(r, hipMemcpyAsync(ws.off + h.m, off.data() + h.m, static_cast<size_t>(len) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_replay_pack, dim3(rs_grid(len)), dim3(kRsBlock), 0, s, rs_ring(r), d, (r->head + first + done + j) % r->cap);
            AO_HIP(r, hipGetLastError());
            const int64_t e0 = done + j;                  // first snapshot entry of the chunk
            AO_HIP(r, hipMemcpyAsync(snap->kind + e0, d.kind, static_cast<size_t>(len), hipMemcpyDeviceToHost, s));
            AO_HIP(r, hipMemcpyAsync(snap->z + e0, d.z, 4 * static_cast<size_t>(len), hipMemcpyDeviceToHost, s));
            AO_HIP(r, hipMemcpyAsync(snap->bits + e0 * h.C * h.W, d.bits, 8 * static_cast<size_t>(len) * h.C * h.W, hipMemcpyDeviceToHost, s));
            AO_HIP(r, hipMemcpyAsync(snap->pi_mask + e0 * h.W, d.mask, 8 * static_cast<size_t>(len) * h.W, hipMemcpyDeviceToHost, s));
            if (npi > 0) AO_HIP(r, hipMemcpyAsync(snap->pi_val + pi_at, d.pival, 8 * static_cast<size_t>(npi), hipMemcpyDeviceToHost, s));
            if (nraw > 0)
                AO_HIP(r, hipMemcpyAsync(snap->raw + raw_at * h.C * h.A, d.raw, static_cast<size_t>(nraw) * h.raw_bytes, hipMemcpyDeviceToHost, s));
            AO_HIP(r, hipStreamSynchronize(s));           // `off` and the workspace are free for the next chunk
            pi_at += npi;
            raw_at += nraw;
            j += len;
        }
        done += blk;
    }
    snap->board = r->B; snap->inplanes = r->C; snap->format = 1; snap->words = h.W;
    snap->entries = n; snap->pi_values = pi_at; snap->raw_entries = raw_at;
    return 0;
}

int ao_replay_import(ao_replay* r, const ao_replay_snapshot* snap, int64_t chunk_bytes, void* stream) {
    using namespace ao;
    if (!snap) return r->fail("ao_replay_import: null snapshot");
    if (chunk_bytes < 0) return r->fail("ao_replay_import: negative chunk_bytes");
    if (snap->board != r->B || snap->inplanes != r->C)
        return r->fail("ao_replay_import: the snapshot is of board " + std::to_string(snap->board) + ", inplanes " + std::to_string(snap->inplanes) +
                       "; the memory has board " + std::to_string(r->B) + ", inplanes " + std::to_string(r->C));
    const std::string why = replay_snapshot_check(snap);
    if (!why.empty()) return r->fail("ao_replay_import: " + why);
    const int64_t E = snap->entries;
    if (E == 0) return 0;
    // deque(maxlen) semantics: only the newest cap entries of the call survive; the slots are those of appending every entry in
    // turn. What survives is at most cap entries with distinct slots, so no launch writes a slot twice.
    const int64_t skip = std::max<int64_t>(0, E - r->cap);
    const RsShape h = rs_shape(r, chunk_bytes, E - skip);
    auto popc = [&](int64_t i) {
        int c = 0;
        for (int w = 0; w < h.W; ++w) c += __builtin_popcountll(snap->pi_mask[i * h.W + w]);
        return c;
    };
    int64_t pi_at = 0, raw_at = 0;
    for (int64_t i = 0; i < skip; ++i) { pi_at += popc(i); raw_at += snap->kind[i]; }
    AO_HIP(r, hipSetDevice(r->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    RsWork ws;
    if (rs_alloc(r, ws, h, true)) return 1;
    const int64_t tail = (r->head + r->count) % r->cap;   // slot of snapshot entry 0
    std::vector<uint32_t> off(2 * static_cast<size_t>(h.m));
    for (int64_t i = skip; i < E;) {
        int64_t len = 0, bytes = 0, npi = 0, nraw = 0;
        while (i + len < E && len < h.m && bytes < h.chunk_bytes) {
            const int nz = popc(i + len), k1 = snap->kind[i + len];
            off[static_cast<size_t>(len)] = static_cast<uint32_t>(npi);
            off[static_cast<size_t>(h.m + len)] = k1 ? static_cast<uint32_t>(nraw) : kNoRaw;
            bytes += h.fixed + 8ll * nz + (k1 ? h.raw_bytes : 0);
            npi += nz;
            nraw += k1;
            ++len;
        }
        const RsLayout l = rs_layout(h, len, npi, nraw);
        const RsChunk d = rs_chunk(ws, h, l, len, npi, nraw);
        AO_HIP(r, hipMemcpyAsync(ws.off, off.data(), static_cast<size_t>(len) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        AO_HIP(r, hipMemcpyAsync(ws.off + h.m, off.data() + h.m, static_cast<size_t>(len) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        AO_HIP(r, hipMemcpyAsync(d.kind, snap->kind + i, static_cast<size_t>(len), hipMemcpyHostToDevice, s));
        AO_HIP(r, hipMemcpyAsync(d.z, snap->z + i, 4 * static_cast<size_t>(len), hipMemcpyHostToDevice, s));
        AO_HIP(r, hipMemcpyAsync(d.bits, snap->bits + i * h.C * h.W, 8 * static_cast<size_t>(len) * h.C * h.W, hipMemcpyHostToDevice, s));
        AO_HIP(r, hipMemcpyAsync(d.mask, snap->pi_mask + i * h.W, 8 * static_cast<size_t>(len) * h.W, hipMemcpyHostToDevice, s));
        if (npi > 0) AO_HIP(r, hipMemcpyAsync(d.pival, snap->pi_val + pi_at, 8 * static_cast<size_t>(npi), hipMemcpyHostToDevice, s));
        if (nraw > 0)
            AO_HIP(r, hipMemcpyAsync(d.raw, snap->raw + raw_at * h.C * h.A, static_cast<size_t>(nraw) * h.raw_bytes, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_replay_unpack, dim3(rs_grid(len)), dim3(kRsBlock), 0, s, rs_ring(r), d, (tail + i % r->cap) % r->cap);
        AO_HIP(r, hipGetLastError());
        AO_HIP(r, hipStreamSynchronize(s));               // `off` and the workspace are free for the next chunk
        pi_at += npi;
        raw_at += nraw;
        i += len;
    }
    const int64_t newcount = std::min<int64_t>(r->cap, r->count + E);
    const int64_t dropped = r->count + E - newcount;
    r->head = (r->head + dropped % r->cap) % r->cap;
    r->count = newcount;
    return 0;
}

}  // extern "C"
