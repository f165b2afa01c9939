// tree_snapshot.hip -- search trees out of the arena and back in: k_tree_pack writes what a game's root reaches as the packed
// arrays of ao_tree_snapshot (include/omok_hip.h), k_tree_unpack builds arena records and positions from them.
//
// k_tree_pack is walk_subtree (tree_walk.hpp: the walk and the numbering of a re-rooting, the root node 0) with stores to the
// snapshot where k_reroot stores to the other arena. It is READ-ONLY on TreeParams: a search that follows an export is bit for
// bit the search without it. k_tree_unpack is the inverse: snapshot node i becomes record i of the game's current arena.
//
// Lanes run over a node's <= 225 edges in NCH chunks of 64; what steers control flow (node, level, counts) is wave-uniform.
#include <cstdint>

#include "host_handle.hpp"
#include "tree_snapshot.hpp"
#include "tree_walk.hpp"

namespace ao {

// ----------------------------------------------------------------------------------------------
// k_tree_pack: table row b = {game, first node, first edge of the game inside the chunk, nodes, edges} as the host sized them
// from k_tree_stats' counts. Every store is bounded by those counts: the trees do not change between the two launches, and a
// tree that did not match would be cut off, not written past its share.
// ----------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(64 * kWalkWaves) void k_tree_pack(TreeParams p, SnapDev d, const int32_t* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    const int32_t* t = table + static_cast<size_t>(blockIdx.x) * kSnapRow;
    const int g = t[0], node_off = t[1], edge_off = t[2], nodes = t[3], edges = t[4];
    if (nodes <= 0 || nodes > p.cap) return;              // (uniform over the workgroup)
    const int lane = lane_id();
    const int root = p.root_node[g];
    if (!link_ok(p, root)) return;
    if (threadIdx.x == 0) {
        d.parent[node_off] = -1;
        d.pedge[node_off] = -1;
    }
    walk_subtree<NCH>(
        p, g, p.cur[g], root, nodes, reinterpret_cast<int32_t*>(s_dyn),
        [](const WalkNode& nd, const PosR&) { return nd.L; },   // nd.before = the node's first edge inside the game
        [&](const WalkNode& nd, int c, int raw, int idx, bool kept) {
            const int e = lane + 64 * c;
            if (c == 0 && lane == 0) d.nchild[node_off + nd.h] = nd.L;    // (h < tail <= nodes)
            if (kept) {
                d.parent[node_off + idx] = nd.h;
                d.pedge[node_off + idx] = e;
            }
            if (e < nd.L && nd.before + e < edges) {
                const size_t at = static_cast<size_t>(edge_off) + nd.before + e;
                d.act[at] = rowACT(p, nd.slot)[e];
                d.n[at] = rowN(p, nd.slot)[e];
                d.w[at] = rowW(p, nd.slot)[e];
                d.q[at] = rowQ(p, nd.slot)[e];
                d.p[at] = rowP(p, nd.slot)[e];
                d.child[at] = kept ? idx : (raw == CH_TERMINAL ? CH_TERMINAL : CH_UNVISITED);
            }
        });
}

// ----------------------------------------------------------------------------------------------
// k_tree_unpack: table row b = {game, first node, first edge inside the chunk, nodes, edges, moves, AO_ROOT_* status, stream
// position}; moves [games][A], mt [games][624]. The host has run snapshot_check (snapshot_check.hpp) and compared nodes with
// keep_max: every parent precedes its children, every offset lies inside the chunk, every record inside the arena.
//
// A record is written as expand_backup_game (tree_device.hpp) leaves it: the six rows for the nchild real edges, the position
// with nchild; the slots nchild..Ap are not written there and not here -- every reader masks by e < nchild.
// Positions: a node's position is its parent's plus the edge's action. Parents precede children and plies do not decrease
// along the order, so level k + 1 -- the expanded children of level k, a contiguous range of node numbers -- needs level k only:
// one barrier per level, the waves of the workgroup taking the nodes of a level in turn.
// An action onto an occupied cell (the host check cannot see it) sets ERR_BAD_MOVE; the host resets that game.
// ----------------------------------------------------------------------------------------------
template <int NCH>
__device__ __forceinline__ int unpack_node(const TreeParams& p, const SnapDev& d, int arena, int g, int node_off, int edge_off, int i,
                                           PosR m) {
    const int lane = lane_id();
    const size_t slot = node_slot(p, arena, g, i);
    const int L = clamp_nchild(p, d.nchild[node_off + i]);
    const size_t fe = static_cast<size_t>(edge_off) + d.first[node_off + i];
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int e = lane + 64 * c;
        int chv = CH_UNVISITED;
        if (e < L) {
            chv = d.child[fe + e];
            rowP(p, slot)[e] = d.p[fe + e];
            rowN(p, slot)[e] = d.n[fe + e];
            rowQ(p, slot)[e] = d.q[fe + e];
            rowCH(p, slot)[e] = chv;
            rowACT(p, slot)[e] = d.act[fe + e];
            rowW(p, slot)[e] = d.w[fe + e];
        }
        cnt += __popcll(__ballot(e < L && chv >= 0));
    }
    if (lane == 0) {
        m.nchild = L;
        pos_store(nodePos(p, slot), m);
    }
    return cnt;
}

template <int NCH>
__global__ __launch_bounds__(64 * kWalkWaves) void k_tree_unpack(TreeParams p, SnapDev d, const int32_t* __restrict__ table,
                                                                 const int32_t* __restrict__ moves_all, const uint32_t* __restrict__ mt_all) {
    __shared__ int32_t s_cnt[kWalkWaves];
    __shared__ int32_t s_bad;
    const int b = blockIdx.x;
    const int32_t* t = table + static_cast<size_t>(b) * kSnapRow;
    const int g = t[0], node_off = t[1], edge_off = t[2], nmoves = t[5], status = t[6], mtpos = t[7];
    const int nodes = (t[3] < 0 || t[3] > p.cap) ? 0 : t[3];   // (the host refused anything above keep_max < cap)
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int arena = p.cur[g];
    for (int i = threadIdx.x; i < 624; i += 64 * kWalkWaves) p.mt[static_cast<size_t>(g) * 624 + i] = mt_all[static_cast<size_t>(b) * 624 + i];
    if (threadIdx.x == 0) s_bad = 0;
    bool bad = false;
    int cnt = 0;
    if (w == 0) {
        // the root position from the move list, as k_walk builds it; then node 0
        const int32_t* mv = moves_all + static_cast<size_t>(b) * p.A;
        PosR rp;
        pos_clear(rp);
        for (int k = 0; k < nmoves && k < p.A; ++k) {
            const int a = mv[k];
            if (a < 0 || a >= p.A || pos_occupied(rp, a)) bad = true;
            else pos_place(rp, a);
        }
        rp.nchild = 0;
        if (lane == 0) {
            pos_store(p.rootpos + g, rp);
            p.mtpos[g] = mtpos;
            p.root_node[g] = nodes > 0 ? 0 : -1;
            p.nodes_used[g] = nodes;
            p.pending_root[g] = 0;
            p.rstatus[g] = status;
            p.gflags[g] = 0;
            p.sims_done[g] = 0;
            p.sims_target[g] = 0;
            p.leaf_status[g] = LS_IDLE;
        }
        if (nodes > 0) cnt = unpack_node<NCH>(p, d, arena, g, node_off, edge_off, 0, rp);
    }
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();
    int lo = 1, hi = 1;
    if (nodes > 0) {
#pragma unroll
        for (int k = 0; k < kWalkWaves; ++k) hi += s_cnt[k];
    }
    hi = hi < nodes ? hi : nodes;
    __syncthreads();
    while (lo < hi) {                                      // (uniform over the workgroup) one level: nodes [lo, hi)
        cnt = 0;
        for (int i = lo + w; i < hi; i += kWalkWaves) {    // (wave-uniform)
            const int par = d.parent[node_off + i], pe = d.pedge[node_off + i];
            const int a = d.act[static_cast<size_t>(edge_off) + d.first[node_off + par] + pe];
            PosR m = pos_load(nodePos(p, node_slot(p, arena, g, par)));   // written one level up, behind a barrier
            if (a >= p.A || pos_occupied(m, a)) bad = true;
            pos_place(m, a);
            cnt += unpack_node<NCH>(p, d, arena, g, node_off, edge_off, i, m);
        }
        if (lane == 0) s_cnt[w] = cnt;
        __syncthreads();                                   // the level's records are visible to the workgroup, the counts are in
        int total = 0;
#pragma unroll
        for (int k = 0; k < kWalkWaves; ++k) total += s_cnt[k];
        lo = hi;
        hi = hi + total < nodes ? hi + total : nodes;
        __syncthreads();
    }
    if (bad && lane == 0) atomicOr(&s_bad, 1);
    __syncthreads();
    if (threadIdx.x == 0) p.err[g] = s_bad ? ERR_BAD_MOVE : 0;
}

// ----------------------------------------------------------------------------------------------
// launchers (called from engine.hip)
// ----------------------------------------------------------------------------------------------

int launch_tree_pack(const TreeParams& p, const SnapDev& d, const int32_t* table, int games, hipStream_t s) {
    const size_t lds = walk_lds_bytes(p.cap);
    if (!lds) return 1;
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_pack<NCH>, dim3(games), dim3(64 * kWalkWaves), lds, s, p, d, table));
    return 0;
}

void launch_tree_unpack(const TreeParams& p, const SnapDev& d, const int32_t* table, const int32_t* moves, const uint32_t* mt, int games,
                        hipStream_t s) {
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_unpack<NCH>, dim3(games), dim3(64 * kWalkWaves), 0, s, p, d, table, moves, mt));
}

}  // namespace ao
