// tree_snapshot.hpp -- what the kernels and the host driver of tree_snapshot.hip share: the layout of one chunk of packed games.
#pragma once
#include "engine_types.hpp"

namespace ao {

// One chunk of a snapshot on the device: the arrays of ao_tree_snapshot (include/omok_hip.h) over the chunk's N nodes and E
// edges, one after the other in ONE buffer so that a chunk is one transfer: the 8-byte array first, the byte array behind the
// 4-byte ones. `first` (a node's first edge inside its game: the running sum of nchild) is host-computed and import-only; it
// lies behind the 25 E + 12 N bytes an export downloads.
struct SnapDev {
    double* p; int32_t* n; float* w; float* q; int32_t* child;   // [E]
    int32_t* nchild; int32_t* parent; int32_t* pedge;            // [N]
    uint8_t* act;                                                // [E]
    int32_t* first;                                              // [N]
};
inline size_t snap_packed_bytes(size_t N, size_t E) { return 25 * E + 12 * N; }
inline size_t snap_dev_bytes(size_t N, size_t E) { return ((snap_packed_bytes(N, E) + 15) & ~static_cast<size_t>(15)) + 4 * N; }
inline SnapDev snap_dev_at(unsigned char* base, size_t N, size_t E) {
    SnapDev d;
    d.p = reinterpret_cast<double*>(base);
    d.n = reinterpret_cast<int32_t*>(base + 8 * E);
    d.w = reinterpret_cast<float*>(base + 12 * E);
    d.q = reinterpret_cast<float*>(base + 16 * E);
    d.child = reinterpret_cast<int32_t*>(base + 20 * E);
    d.nchild = reinterpret_cast<int32_t*>(base + 24 * E);
    d.parent = d.nchild + N;
    d.pedge = d.parent + N;
    d.act = base + 24 * E + 12 * N;
    d.first = reinterpret_cast<int32_t*>(base + ((snap_packed_bytes(N, E) + 15) & ~static_cast<size_t>(15)));
    return d;
}

// a chunk's game table, kSnapRow int32 per game: engine slot, first node and first edge inside the chunk, nodes, edges, and for
// the import the number of moves, the AO_ROOT_* status and the stream position
constexpr int kSnapRow = 8;

}  // namespace ao
