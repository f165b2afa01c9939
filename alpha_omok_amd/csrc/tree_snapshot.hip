// tree_snapshot.hip -- search trees out of the arena and back in: k_tree_pack writes what a game's root reaches as the packed
// arrays of ao_tree_snapshot (include/omok_hip.h), k_tree_unpack builds arena records and positions from them.
//
// k_tree_pack is walk_subtree (tree_walk.hpp: the walk and the numbering of a re-rooting, the root node 0) with stores to the
// snapshot where k_reroot stores to the other arena. It is READ-ONLY on TreeParams: a search that follows an export is bit for
// bit the search without it. k_tree_unpack is the inverse: snapshot node i becomes record i of the game's current arena.
//
// Lanes run over a node's <= 225 edges in NCH chunks of 64; what steers control flow (node, level, counts) is wave-uniform.
//
// The host side (ao_tree_export, ao_tree_snapshot_check, ao_tree_import) follows the kernels: the games of a call travel in chunks
// of bounded size through the engine's read-out workspace, each chunk laid out by tree_snapshot.hpp.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "snapshot_check.hpp"
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
// launchers
// ----------------------------------------------------------------------------------------------

// non-zero: the breadth-first queue of a `cap`-node arena does not fit the LDS of one workgroup -- nothing is launched
static int launch_tree_pack(const TreeParams& p, const SnapDev& d, const int32_t* table, int games, hipStream_t s) {
    const size_t lds = walk_lds_bytes(p.cap);
    if (!lds) return 1;
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_pack<NCH>, dim3(games), dim3(64 * kWalkWaves), lds, s, p, d, table));
    return 0;
}

static void launch_tree_unpack(const TreeParams& p, const SnapDev& d, const int32_t* table, const int32_t* moves, const uint32_t* mt, int games,
                               hipStream_t s) {
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_unpack<NCH>, dim3(games), dim3(64 * kWalkWaves), 0, s, p, d, table, moves, mt));
}

}  // namespace ao

// ----------------------------------------------------------------------------------------------
// the host side: export, check, import
// ----------------------------------------------------------------------------------------------
// games of one chunk: [first, first + count) of the call's list, N nodes and E edges together
struct SnapChunk { int first, count; size_t N, E; };

// closes a chunk when its packed games reach kSnapChunkBytes (a chunk holds at least one game): the device workspace is
// bounded by that plus one game, whatever node_cap is
static std::vector<SnapChunk> snap_chunks(const std::vector<int32_t>& nodes, const std::vector<int32_t>& edges) {
    constexpr size_t kSnapChunkBytes = static_cast<size_t>(64) << 20;
    std::vector<SnapChunk> out;
    SnapChunk c{0, 0, 0, 0};
    for (int i = 0; i < static_cast<int>(nodes.size()); ++i) {
        c.count += 1;
        c.N += static_cast<size_t>(nodes[i]);
        c.E += static_cast<size_t>(edges[i]);
        if (ao::snap_packed_bytes(c.N, c.E) >= kSnapChunkBytes) {
            out.push_back(c);
            c = SnapChunk{i + 1, 0, 0, 0};
        }
    }
    if (c.count > 0) out.push_back(c);
    return out;
}

// workspace of a chunk: the packed arrays (+ `first`), the game table, and for an import the moves and the streams
static size_t snap_table_at(const SnapChunk& c) { return (ao::snap_dev_bytes(c.N, c.E) + 15) & ~static_cast<size_t>(15); }
static size_t snap_chunk_bytes(const SnapChunk& c, int A, bool import) {
    return snap_table_at(c) + static_cast<size_t>(c.count) * 4 * (ao::kSnapRow + (import ? A + 624 : 0));
}

extern "C" {

int ao_tree_export(ao_engine* e, const uint8_t* mask, ao_tree_snapshot* out) {
    if (roll_refuses(e, "ao_tree_export")) return 1;
    if (e->in_move) return e->fail("ao_tree_export inside a move (between ao_begin_move and ao_end_move)");
    if (!out) return e->fail("ao_tree_export: null snapshot");
    const int G = e->G, A = e->A;
    std::vector<int32_t> games;
    for (int g = 0; g < G; ++g)
        if (!mask || mask[g]) games.push_back(g);
    const int ng = static_cast<int>(games.size());
    if (ng > 0 && (!out->hdr || !out->gauss || !out->mt || !out->moves)) return e->fail("ao_tree_export: null hdr / gauss / mt / moves array");
    // one stats pass: what every masked game's root reaches
    std::vector<int32_t> st(static_cast<size_t>(G) * 4, 0);
    if (ao_tree_stats(e, mask, st.data())) return 1;
    std::vector<int32_t> nodes(ng), edges(ng);
    int64_t N = 0, E = 0;
    for (int i = 0; i < ng; ++i) {
        const int32_t* s4 = st.data() + 4 * static_cast<size_t>(games[i]);
        nodes[i] = s4[0];
        edges[i] = s4[0] > 0 ? s4[1] - 1 : 0;
        N += nodes[i];
        E += edges[i];
    }
    if (N > out->nodes || E > out->edges)
        return e->fail("ao_tree_export: the masked games hold " + std::to_string(N) + " nodes and " + std::to_string(E) + " edges, the snapshot's arrays " +
                       std::to_string(out->nodes) + " and " + std::to_string(out->edges));
    if (N > 0 && (!out->nchild || !out->parent || !out->parent_edge)) return e->fail("ao_tree_export: null node array");
    if (E > 0 && (!out->act || !out->n || !out->w || !out->q || !out->p || !out->child)) return e->fail("ao_tree_export: null edge array");
    const std::vector<SnapChunk> chunks = snap_chunks(nodes, edges);
    size_t ws = 0;
    for (const SnapChunk& c : chunks) ws = std::max(ws, snap_chunk_bytes(c, A, false));
    if (readout_begin(e, "ao_tree_export", ws)) return 1;
    size_t n0 = 0, e0 = 0;   // first node / edge of the chunk in the caller's arrays
    for (const SnapChunk& c : chunks) {
        if (c.N == 0) continue;
        const size_t tab_at = snap_table_at(c);
        int32_t* h_tab = reinterpret_cast<int32_t*>(e->h_ro.data() + tab_at);
        size_t no = 0, eo = 0;
        for (int k = 0; k < c.count; ++k) {
            int32_t* row = h_tab + static_cast<size_t>(k) * ao::kSnapRow;
            const int i = c.first + k;
            row[0] = games[i]; row[1] = static_cast<int32_t>(no); row[2] = static_cast<int32_t>(eo); row[3] = nodes[i]; row[4] = edges[i];
            row[5] = row[6] = row[7] = 0;
            no += nodes[i];
            eo += edges[i];
        }
        const ao::SnapDev d = ao::snap_dev_at(e->d_ro.p, c.N, c.E);
        AO_HIP(e, hipMemcpyAsync(e->d_ro.p + tab_at, h_tab, static_cast<size_t>(c.count) * ao::kSnapRow * 4, hipMemcpyHostToDevice, e->stream));
        if (ao::launch_tree_pack(e->tp, d, reinterpret_cast<const int32_t*>(e->d_ro.p + tab_at), c.count, e->stream))
            return queue_refused(e, "ao_tree_export");
        AO_HIP(e, hipGetLastError());
        AO_HIP(e, hipMemcpyAsync(e->h_ro.data(), e->d_ro.p, ao::snap_packed_bytes(c.N, c.E), hipMemcpyDeviceToHost, e->stream));
        AO_HIP(e, hipStreamSynchronize(e->stream));   // the staging buffers are reused by the next chunk
        const ao::SnapDev h = ao::snap_dev_at(e->h_ro.data(), c.N, c.E);
        std::memcpy(out->p + e0, h.p, 8 * c.E);
        std::memcpy(out->n + e0, h.n, 4 * c.E);
        std::memcpy(out->w + e0, h.w, 4 * c.E);
        std::memcpy(out->q + e0, h.q, 4 * c.E);
        std::memcpy(out->child + e0, h.child, 4 * c.E);
        std::memcpy(out->act + e0, h.act, c.E);
        std::memcpy(out->nchild + n0, h.nchild, 4 * c.N);
        std::memcpy(out->parent + n0, h.parent, 4 * c.N);
        std::memcpy(out->parent_edge + n0, h.pedge, 4 * c.N);
        n0 += c.N;
        e0 += c.E;
    }
    // the streams (the pinned staging rows of ao_begin_move are free outside a move) and the host mirrors
    AO_HIP(e, hipMemcpyAsync(e->h_mt, e->tp.mt, sizeof(uint32_t) * 624 * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipMemcpyAsync(e->h_pos, e->tp.mtpos, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    for (int i = 0; i < ng; ++i) {
        const int g = games[i];
        int32_t* h = out->hdr + static_cast<size_t>(i) * AO_SNAP_HDR;
        h[0] = nodes[i]; h[1] = edges[i]; h[2] = static_cast<int32_t>(e->moves[g].size()); h[3] = e->status[g]; h[4] = e->over[g];
        h[5] = e->h_pos[g]; h[6] = e->has_gauss[g]; h[7] = 0;
        out->gauss[i] = e->gauss[g];
        std::memcpy(out->mt + static_cast<size_t>(i) * 624, e->h_mt + static_cast<size_t>(g) * 624, sizeof(uint32_t) * 624);
        int32_t* mv = out->moves + static_cast<size_t>(i) * A;
        std::fill(mv, mv + A, 0);
        std::copy(e->moves[g].begin(), e->moves[g].end(), mv);
    }
    out->board = e->cfg.board; out->inplanes = e->cfg.inplanes; out->win_mark = e->tp.win_mark;
    out->sims = e->S; out->noise = e->tp.noise; out->c_puct = e->tp.c_puct;
    out->games = ng; out->nodes = N; out->edges = E;
    return 0;
}

int ao_tree_snapshot_check(const ao_tree_snapshot* snap) {
    std::string& why = ao::create_error<ao_engine>();
    why = ao::snapshot_check(snap);
    return why.empty() ? 0 : 1;
}

int ao_tree_import(ao_engine* e, const int32_t* host_games, int32_t n, const ao_tree_snapshot* snap) {
    if (roll_refuses(e, "ao_tree_import")) return 1;
    if (e->in_move) return e->fail("ao_tree_import inside a move (between ao_begin_move and ao_end_move)");
    if (!snap || (n > 0 && !host_games)) return e->fail("ao_tree_import: null argument");
    if (n != snap->games) return e->fail("ao_tree_import: " + std::to_string(n) + " games listed, the snapshot holds " + std::to_string(snap->games));
    const int G = e->G, A = e->A;
    std::vector<uint8_t> seen(G, 0);
    for (int i = 0; i < n; ++i) {
        if (host_games[i] < 0 || host_games[i] >= G) return e->fail("game index out of range");
        if (seen[host_games[i]]) return e->fail("ao_tree_import: a game is listed twice");
        seen[host_games[i]] = 1;
    }
    if (snap->board != e->cfg.board || snap->inplanes != e->cfg.inplanes || snap->win_mark != e->tp.win_mark)
        return e->fail("ao_tree_import: the snapshot is of board " + std::to_string(snap->board) + ", inplanes " + std::to_string(snap->inplanes) +
                       ", win_mark " + std::to_string(snap->win_mark) + "; the engine has board " + std::to_string(e->cfg.board) + ", inplanes " +
                       std::to_string(e->cfg.inplanes) + ", win_mark " + std::to_string(e->tp.win_mark));
    const std::string why = ao::snapshot_check(snap);
    if (!why.empty()) return e->fail("ao_tree_import: inconsistent snapshot: " + why);
    if (n == 0) return 0;
    // a pending bar belongs to the position it was set for; a snapshot taken after a barred move brings kBarQ children with it
    std::vector<uint8_t> listed(G, 0);
    for (int i = 0; i < n; ++i) listed[host_games[i]] = 1;
    if (bar_forget(e, listed.data())) return 1;
    for (int64_t k = 0; k < snap->edges && !e->bar_dirty; ++k) e->bar_dirty = snap->q[k] == ao::kBarQ;
    std::vector<int32_t> nodes(n), edges(n);
    for (int i = 0; i < n; ++i) {
        nodes[i] = snap->hdr[static_cast<size_t>(i) * AO_SNAP_HDR];
        edges[i] = snap->hdr[static_cast<size_t>(i) * AO_SNAP_HDR + 1];
        if (nodes[i] > e->tp.keep_max)
            return e->fail("ao_tree_import: snapshot game " + std::to_string(i) + " has " + std::to_string(nodes[i]) + " nodes, this engine keeps at most node_cap - sims - 1 = " +
                           std::to_string(e->tp.keep_max) + " (raise ao_config.node_cap)");
    }
    const std::vector<SnapChunk> chunks = snap_chunks(nodes, edges);
    size_t ws = 0;
    for (const SnapChunk& c : chunks) ws = std::max(ws, snap_chunk_bytes(c, A, true));
    if (readout_begin(e, "ao_tree_import", ws)) return 1;
    size_t n0 = 0, e0 = 0;
    for (const SnapChunk& c : chunks) {
        AO_HIP(e, hipStreamSynchronize(e->stream));   // the staging buffer is free
        const ao::SnapDev h = ao::snap_dev_at(e->h_ro.data(), c.N, c.E);
        std::memcpy(h.p, snap->p + e0, 8 * c.E);
        std::memcpy(h.n, snap->n + e0, 4 * c.E);
        std::memcpy(h.w, snap->w + e0, 4 * c.E);
        std::memcpy(h.q, snap->q + e0, 4 * c.E);
        std::memcpy(h.child, snap->child + e0, 4 * c.E);
        std::memcpy(h.act, snap->act + e0, c.E);
        std::memcpy(h.nchild, snap->nchild + n0, 4 * c.N);
        std::memcpy(h.parent, snap->parent + n0, 4 * c.N);
        std::memcpy(h.pedge, snap->parent_edge + n0, 4 * c.N);
        const size_t tab_at = snap_table_at(c);
        int32_t* h_tab = reinterpret_cast<int32_t*>(e->h_ro.data() + tab_at);
        int32_t* h_mv = h_tab + static_cast<size_t>(c.count) * ao::kSnapRow;
        uint32_t* h_mt = reinterpret_cast<uint32_t*>(h_mv + static_cast<size_t>(c.count) * A);
        size_t no = 0, eo = 0;
        for (int k = 0; k < c.count; ++k) {
            const int i = c.first + k;
            const int32_t* hd = snap->hdr + static_cast<size_t>(i) * AO_SNAP_HDR;
            int32_t* row = h_tab + static_cast<size_t>(k) * ao::kSnapRow;
            row[0] = host_games[i]; row[1] = static_cast<int32_t>(no); row[2] = static_cast<int32_t>(eo); row[3] = nodes[i]; row[4] = edges[i];
            row[5] = hd[2]; row[6] = hd[3]; row[7] = hd[5];
            int32_t run = 0;   // a node's first edge inside its game
            for (int j = 0; j < nodes[i]; ++j) {
                h.first[no + j] = run;
                run += h.nchild[no + j];
            }
            std::memcpy(h_mv + static_cast<size_t>(k) * A, snap->moves + static_cast<size_t>(i) * A, sizeof(int32_t) * A);
            std::memcpy(h_mt + static_cast<size_t>(k) * 624, snap->mt + static_cast<size_t>(i) * 624, sizeof(uint32_t) * 624);
            no += nodes[i];
            eo += edges[i];
        }
        const size_t bytes = snap_chunk_bytes(c, A, true);
        AO_HIP(e, hipMemcpyAsync(e->d_ro.p, e->h_ro.data(), bytes, hipMemcpyHostToDevice, e->stream));
        const int32_t* d_tab = reinterpret_cast<const int32_t*>(e->d_ro.p + tab_at);
        const int32_t* d_mv = d_tab + static_cast<size_t>(c.count) * ao::kSnapRow;
        ao::launch_tree_unpack(e->tp, ao::snap_dev_at(e->d_ro.p, c.N, c.E), d_tab, d_mv,
                               reinterpret_cast<const uint32_t*>(d_mv + static_cast<size_t>(c.count) * A), c.count, e->stream);
        AO_HIP(e, hipGetLastError());
        n0 += c.N;
        e0 += c.E;
    }
    int32_t* herr = e->h_i32;
    AO_HIP(e, hipMemcpyAsync(herr, e->tp.err, sizeof(int32_t) * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    std::vector<uint8_t> bmask;
    std::string bad;
    for (int i = 0; i < n; ++i) {
        const int g = host_games[i];
        const int32_t* hd = snap->hdr + static_cast<size_t>(i) * AO_SNAP_HDR;
        const int32_t* mv = snap->moves + static_cast<size_t>(i) * A;
        e->moves[g].assign(mv, mv + hd[2]);
        e->status[g] = hd[3];
        e->over[g] = hd[4];
        e->has_gauss[g] = hd[6];
        e->gauss[g] = snap->gauss[i];
        if (herr[g] & ao::ERR_BAD_MOVE) {
            if (bmask.empty()) bmask.assign(G, 0);
            bmask[g] = 1;
            bad += (bad.empty() ? "" : ", ") + std::to_string(i);
        }
    }
    e->ended = false;   // ao_play must follow a search on this engine, as on a fresh one
    if (!bmask.empty()) {
        ao_reset(e, bmask.data());
        return e->fail("ao_tree_import: snapshot game(s) " + bad + ": an action lands on an occupied cell when the positions are rebuilt; reset (the other games of the call are imported)");
    }
    return 0;
}

}  // extern "C"
