// tree_walk.hpp -- the ONE breadth-first walk over what a node of a game's arena reaches, and the small device helpers every
// kernel that follows links of the tree shares. Included by tree_kernels.hip (k_reroot copies the walked subtree into the other
// arena; k_play, k_walk), tree_readout.hip (k_tree_stats counts it; k_tree_lookup, k_tree_pv) and tree_snapshot.hip (k_tree_pack
// stores it into a snapshot).
//
// The numbering is the contract: the walk's root is node 0, the followable children get the next numbers in queue order, within a
// node in stored edge order, and a child is kept (walked in its turn) if and only if its number is below `limit`. A snapshot's
// node i is a re-rooting's node i, and the import (k_tree_unpack) relies on it.
#pragma once
#include <type_traits>

#include "tree_device.hpp"

namespace ao {

constexpr int kWalkWaves = 8;                  // waves of a walking workgroup: the record reads of that many nodes are in flight together
constexpr int kWalkHdr = 3 * kWalkWaves;       // int32 words in front of the queue: the walk's two per-wave blocks + one more for the caller's epilogue
constexpr size_t kWalkMaxLds = 64 * 1024;      // dynamic LDS a launch gets without opting in to more

// Dynamic LDS of a walk inside a `cap`-node arena: the header and a queue that holds every node; 0 = it does not fit, launch
// nothing. ao_create refuses node_cap > 15000 and 4 * 15000 + 96 B < 64 KiB: no launch of an engine that exists is refused.
inline size_t walk_lds_bytes(int cap) {
    const size_t b = (kWalkHdr + static_cast<size_t>(cap)) * 4;
    return b <= kWalkMaxLds ? b : 0;
}

// a child link that can be followed: an expanded child inside the arena (anything else in a consistent tree is CH_UNVISITED / CH_TERMINAL)
__device__ __forceinline__ bool link_ok(const TreeParams& p, int ch) { return ch >= 0 && ch < p.cap; }

// a stored child count as every reader uses it: inside [0, A]
__device__ __forceinline__ int clamp_nchild(const TreeParams& p, int L) { return L < 0 ? 0 : (L > p.A ? p.A : L); }
__device__ __forceinline__ int node_nchild(const TreeParams& p, size_t slot) { return clamp_nchild(p, pos_load(nodePos(p, slot)).nchild); }

// stored index of the edge of `slot` that plays `a`, -1 if there is none (an occupied or off-board cell has no edge)
template <int NCH>
__device__ __forceinline__ int find_edge(const TreeParams& p, size_t slot, int L, int a) {
    const int lane = lane_id();
    const uint8_t* rACT = rowACT(p, slot);
    int found = -1;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int e = lane + 64 * c;
        const int ec = e < p.Ap ? e : p.Ap - 1;
        const uint64_t mk = __ballot(e < L && static_cast<int>(rACT[ec]) == a);
        if (found < 0 && mk) found = 64 * c + __ffsll(static_cast<long long>(mk)) - 1;
    }
    return found;
}

// the node a wave holds in one round: queue entry h (= its new number), its record, its clamped child count, and `before`: the
// sum of what on_node returned for the queue entries in front of it (0 if on_node returns nothing)
struct WalkNode { int h; size_t slot; int L; int before; };
struct WalkEnd { int tail; bool over; };   // nodes walked (<= limit); the tree reaches more than `limit`

// One workgroup of kWalkWaves waves walks what `root` reaches in `arena` of game g; `lds` = walk_lds_bytes(p.cap) bytes. Wave w
// takes queue entry head + w; the children's numbers come from a prefix over the waves' child counts in queue order.
//   on_node(node, m)                      before the round's barrier: the wave has its node and its position record m. Whatever else the
//                                         caller loads here is in flight together with the other waves' reads. It may return an int,
//                                         which the walk sums over the queue order into WalkNode::before (two more LDS words per
//                                         wave and round); returning void costs nothing.
//   on_edges(node, c, raw, idx, kept)     after the numbering, once per chunk c of 64 edges (lane's edge e = lane + 64 c, c a
//                                         compile-time constant after unrolling): the stored link, the child's number (-1: not
//                                         followable or e >= L), and whether it is walked (idx >= 0 && idx < limit).
// Both are called by the waves that have a node only; everything that steers control flow is wave-uniform.
template <int NCH, class OnNode, class OnEdges>
__device__ __forceinline__ WalkEnd walk_subtree(const TreeParams& p, int g, int arena, int root, int limit, int32_t* lds,
                                                OnNode&& on_node, OnEdges&& on_edges) {
    using NodeSum = decltype(on_node(WalkNode{}, PosR{}));
    constexpr bool kSums = !std::is_void<NodeSum>::value;
    int32_t* s_cnt = lds;                    // [kWalkWaves] followable children each wave's node brings
    int32_t* s_sum = lds + kWalkWaves;       // [kWalkWaves] what on_node returned
    int32_t* s_q = lds + kWalkHdr;           // [cap] the queue: arena index of the node that becomes number i
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_q[0] = root;
    __syncthreads();
    int tail = 1, sums = 0;
    bool over = false;
    for (int head = 0; head < tail;) {
        WalkNode nd{head + w, 0, 0, sums};
        const bool have = nd.h < tail;       // (wave-uniform) this round takes queue entries [head, min(head + waves, tail))
        const int next_head = head + kWalkWaves < tail ? head + kWalkWaves : tail;
        int raw[NCH];
        bool ok[NCH];
        int cnt = 0, mine = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) { raw[c] = CH_UNVISITED; ok[c] = false; }
        if (have) {
            nd.slot = node_slot(p, arena, g, s_q[nd.h]);
            const PosR m = pos_load(nodePos(p, nd.slot));
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int e = lane + 64 * c;
                raw[c] = rowCH(p, nd.slot)[e < p.Ap ? e : p.Ap - 1];
            }
            nd.L = clamp_nchild(p, m.nchild);
            if constexpr (kSums) mine = on_node(nd, m);
            else on_node(nd, m);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                ok[c] = lane + 64 * c < nd.L && link_ok(p, raw[c]);
                cnt += __popcll(__ballot(ok[c]));
            }
        }
        if (lane == 0) {
            s_cnt[w] = cnt;
            if constexpr (kSums) s_sum[w] = mine;
        }
        __syncthreads();
        int base = tail, total = 0;
#pragma unroll
        for (int k = 0; k < kWalkWaves; ++k) {
            const int ck = s_cnt[k];
            if (k < w) base += ck;
            total += ck;
            if constexpr (kSums) {
                const int sk = s_sum[k];
                if (k < w) nd.before += sk;
                sums += sk;
            }
        }
        if (have) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint64_t mk = __ballot(ok[c]);
                const int idx = ok[c] ? base + __popcll(mk & lanes_below()) : -1;
                const bool kept = ok[c] && idx < limit;
                if (kept) s_q[idx] = raw[c];
                on_edges(nd, c, raw[c], idx, kept);
                base += __popcll(mk);
            }
        }
        // (numbers are handed out in queue order: everything below `limit` is kept, so the queue grows by what fits)
        over = over || tail + total > limit;
        tail = tail + total < limit ? tail + total : limit;
        head = next_head;
        __syncthreads();
    }
    return WalkEnd{tail, over};
}

}  // namespace ao
