// tree_readout.hip -- reading the search trees where they live: node lookup by id, principal variations and tree statistics
// for all games in one launch each, O(result) bytes back to the host. Every kernel here is READ-ONLY on TreeParams, so a search
// that follows a read-out is bit for bit the search that would have run without it. They share their steps with the kernels that
// write (tree_walk.hpp): find_edge (id -> node, as k_walk) and walk_subtree (the breadth-first walk of k_reroot).
//
// Reference map (paths relative to the reference's 2_AlphaOmok/):
//   k_tree_lookup   agents.py:52,206-210  self.tree[node_id] -> {'child', 'n', 'w', 'q', 'p'} for n ids at once. The engine keeps a
//                                         node's n / w / q / p on its PARENT's edge (engine_types.hpp), the children in stored order
//                                         (utils.legal_actions order, agents.py:182,212) in the node's own record.
//   k_tree_pv       (no counterpart)      the line of most-visited edges from the root: what argmax over agents.py:67-69 gives when
//                                         it is applied again and again; first maximum in stored order.
//   k_tree_stats    agents.py:241-250     del_parents' `tree size` / `tree depth` prints for the subtree the root reaches, plus how
//                                         much of the arena that subtree occupies.
//
// One wavefront per query / per game (k_tree_lookup, k_tree_pv: kReadPerWG of them per workgroup, nothing shared, no barrier);
// k_tree_stats: one workgroup of kWalkWaves waves per game. Lanes run over a node's <= 225 edges in NCH chunks of 64; everything
// that steers control flow (game, move, edge found, child link) is wave-uniform: ballots, readfirstlane, DPP reductions.
#include <cstdint>

#include "../../include/omok_hip.h"
#include "host_handle.hpp"
#include "launchers.hpp"
#include "tree_walk.hpp"

namespace ao {

constexpr int kReadPerWG = 4;

// ----------------------------------------------------------------------------------------------
// k_tree_lookup: query i = (game, m moves beyond that game's root). Row i of `queries`: game, m (< 0: the id does not extend
// the root -- the host compared the prefix), root_known (the root is a key although it has no record: AO_ROOT_UNEXPANDED), moves.
// ----------------------------------------------------------------------------------------------
struct LookupOut {
    int32_t* status; int32_t* nchild; double* nwqp;                         // [n], [n], [n][4]
    int32_t* c_act; int32_t* c_n; float* c_w; float* c_q; double* c_p;      // [n][A] each, or all null
};

template <int NCH>
__global__ __launch_bounds__(64 * kReadPerWG) void k_tree_lookup(TreeParams p, const int32_t* __restrict__ queries, int n, int stride,
                                                                 LookupOut o) {
    const int i = blockIdx.x * kReadPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (i >= n) return;
    const int lane = lane_id();
    const int32_t* qr = queries + static_cast<size_t>(i) * stride;
    const int g = __builtin_amdgcn_readfirstlane(qr[0]);
    const int m = __builtin_amdgcn_readfirstlane(qr[1]);
    const int root_known = __builtin_amdgcn_readfirstlane(qr[2]);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int arena = p.cur[g];
    int node = p.root_node[g];
    if (!link_ok(p, node)) node = -1;
    int status = m < 0 ? AO_NODE_ABSENT : (node >= 0 ? AO_NODE_EXPANDED : (root_known ? AO_NODE_LEAF : AO_NODE_ABSENT));
    double own_n = nan, own_w = nan, own_q = nan, own_p = nan;
    for (int k = 0; k < m && status != AO_NODE_ABSENT; ++k) {
        const int a = __builtin_amdgcn_readfirstlane(qr[3 + k]);
        if (status != AO_NODE_EXPANDED || a < 0 || a >= p.A) { status = AO_NODE_ABSENT; break; }   // the children of a leaf are no keys
        const size_t slot = node_slot(p, arena, g, node);
        const int found = find_edge<NCH>(p, slot, node_nchild(p, slot), a);
        if (found < 0) { status = AO_NODE_ABSENT; break; }
        const int ch = rowCH(p, slot)[found];
        own_n = static_cast<double>(rowN(p, slot)[found]);
        own_w = static_cast<double>(rowW(p, slot)[found]);
        own_q = static_cast<double>(rowQ(p, slot)[found]);
        own_p = rowP(p, slot)[found];
        if (link_ok(p, ch)) node = ch;
        else status = ch == CH_TERMINAL ? AO_NODE_TERMINAL : AO_NODE_LEAF;
    }
    if (status == AO_NODE_ABSENT) own_n = own_w = own_q = own_p = nan;
    int L = 0;
    int cn[NCH], ca[NCH];
    float cw[NCH], cq[NCH];
    double cp[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) { cn[c] = 0; ca[c] = -1; cw[c] = 0.f; cq[c] = 0.f; cp[c] = 0.0; }
    if (status == AO_NODE_EXPANDED) {
        const size_t slot = node_slot(p, arena, g, node);
        L = node_nchild(p, slot);
        int tot = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int e = lane + 64 * c;
            const int ec = e < p.Ap ? e : p.Ap - 1;
            const int vn = rowN(p, slot)[ec], va = rowACT(p, slot)[ec];
            const float vw = rowW(p, slot)[ec], vq = rowQ(p, slot)[ec];
            const double vp = rowP(p, slot)[ec];
            if (e < L) { cn[c] = vn; ca[c] = va; cw[c] = vw; cq[c] = vq; cp[c] = vp; }
            tot += cn[c];
        }
        // the root has no parent edge: the simulation that expanded it visited no child, every later one exactly one
        if (m == 0) own_n = static_cast<double>(1 + wave_sum_i(tot));
    }
    if (lane == 0) {
        o.status[i] = status;
        o.nchild[i] = L;
        o.nwqp[4 * static_cast<size_t>(i) + 0] = own_n;
        o.nwqp[4 * static_cast<size_t>(i) + 1] = own_w;
        o.nwqp[4 * static_cast<size_t>(i) + 2] = own_q;
        o.nwqp[4 * static_cast<size_t>(i) + 3] = own_p;
    }
    if (o.c_act) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int e = lane + 64 * c;
            if (e >= p.A) continue;
            const size_t at = static_cast<size_t>(i) * p.A + e;
            o.c_act[at] = ca[c];
            o.c_n[at] = cn[c];
            o.c_w[at] = cw[c];
            o.c_q[at] = cq[c];
            o.c_p[at] = cp[c];
        }
    }
}

// ----------------------------------------------------------------------------------------------
// k_tree_pv: from the root, the edge with the most visits, ties to the lowest stored index (a ballot + first set bit, as the
// selection picks: deterministic). Ends when the best n is 0, behind an edge whose child is not expanded, or at max_len.
// Rows of games with mask[g] == 0 are not written.
// ----------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(64 * kReadPerWG) void k_tree_pv(TreeParams p, const uint8_t* __restrict__ mask, int max_len, int32_t* out_act,
                                                             int32_t* out_n, float* out_q, int32_t* out_len) {
    const int g = blockIdx.x * kReadPerWG + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (g >= p.G) return;
    if (!mask[g]) return;
    const int lane = lane_id();
    const int arena = p.cur[g];
    int node = p.root_node[g];
    int len = 0;
    while (link_ok(p, node) && len < max_len) {
        const size_t slot = node_slot(p, arena, g, node);
        const int L = node_nchild(p, slot);
        int nv[NCH];
        int best = -1;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int e = lane + 64 * c;
            const int ec = e < p.Ap ? e : p.Ap - 1;
            const int v = rowN(p, slot)[ec];
            nv[c] = e < L ? v : -1;
            best = nv[c] > best ? nv[c] : best;
        }
        best = wave_max_i(best);
        if (best <= 0) break;
        int esel = -1;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint64_t mk = __ballot(nv[c] == best);
            if (esel < 0 && mk) esel = 64 * c + __ffsll(static_cast<long long>(mk)) - 1;
        }
        const int ch = rowCH(p, slot)[esel];
        if (lane == 0) {
            const size_t at = static_cast<size_t>(g) * max_len + len;
            out_act[at] = rowACT(p, slot)[esel];
            out_n[at] = best;
            out_q[at] = rowQ(p, slot)[esel];
        }
        ++len;
        node = ch;
    }
    if (lane == 0) out_len[g] = len;
}

// ----------------------------------------------------------------------------------------------
// k_tree_stats: walk_subtree (tree_walk.hpp) over what the root reaches, inside the whole arena (limit = cap); counts are
// accumulated where k_reroot copies records.
// mask[g]: 0 = skip the game, 1 = its root is not a key (fresh), 2 = its root is a key. out[g] = {expanded nodes reachable from
// the root, dict entries (1 + sum of nchild over them), depth, nodes_used}; depth = the largest ply + (nchild > 0) over the
// reachable expanded nodes (the longest key of the reference's dict, minus one: agents.py:241-250), the root's ply if the root
// is only known, 0 without a tree. A tree that reaches more than `cap` nodes cannot exist: expanded = -1 reports it.
// ----------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(64 * kWalkWaves) void k_tree_stats(TreeParams p, const uint8_t* __restrict__ mask, int32_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    int32_t* lds = reinterpret_cast<int32_t*>(s_dyn);
    const int g = blockIdx.x;
    const int mk_g = mask[g];
    if (mk_g == 0) return;                                // (uniform over the workgroup)
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int root = p.root_node[g];
    if (!link_ok(p, root)) {
        if (threadIdx.x == 0) {
            out[4 * g + 0] = 0;
            out[4 * g + 1] = 0;
            out[4 * g + 2] = mk_g == 2 ? static_cast<int>(p.rootpos[g].ply) : 0;
            out[4 * g + 3] = p.nodes_used[g];
        }
        return;
    }
    int entries = 0, depth = 0;
    const WalkEnd end = walk_subtree<NCH>(
        p, g, p.cur[g], root, p.cap, lds,
        [&](const WalkNode& nd, const PosR& m) {
            entries += nd.L;
            const int d = m.ply + (nd.L > 0 ? 1 : 0);
            depth = d > depth ? d : depth;
        },
        [](const WalkNode&, int, int, int, bool) {});
    if (lane == 0) { lds[w] = entries; lds[kWalkWaves + w] = depth; }   // (behind the walk's last barrier: the header is free)
    __syncthreads();
    if (threadIdx.x == 0) {
        int en = 1, dp = 0;
        for (int k = 0; k < kWalkWaves; ++k) {
            en += lds[k];
            dp = lds[kWalkWaves + k] > dp ? lds[kWalkWaves + k] : dp;
        }
        out[4 * g + 0] = end.over ? -1 : end.tail;
        out[4 * g + 1] = en;
        out[4 * g + 2] = dp;
        out[4 * g + 3] = p.nodes_used[g];
    }
}

// ----------------------------------------------------------------------------------------------
// launchers (called from engine.hip)
// ----------------------------------------------------------------------------------------------

void launch_tree_lookup(const TreeParams& p, const int32_t* queries, int n, int stride, int32_t* status, int32_t* nchild, double* nwqp,
                        int32_t* c_act, int32_t* c_n, float* c_w, float* c_q, double* c_p, hipStream_t s) {
    const LookupOut o{status, nchild, nwqp, c_act, c_n, c_w, c_q, c_p};
    const dim3 grid(static_cast<unsigned>((n + kReadPerWG - 1) / kReadPerWG)), block(64 * kReadPerWG);
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_lookup<NCH>, grid, block, 0, s, p, queries, n, stride, o));
}

void launch_tree_pv(const TreeParams& p, const uint8_t* mask, int max_len, int32_t* act, int32_t* n, float* q, int32_t* len, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((p.G + kReadPerWG - 1) / kReadPerWG)), block(64 * kReadPerWG);
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_pv<NCH>, grid, block, 0, s, p, mask, max_len, act, n, q, len));
}

// non-zero: the queue of a `cap`-node arena does not fit the LDS of one workgroup (walk_lds_bytes) -- nothing is launched
int launch_tree_stats(const TreeParams& p, const uint8_t* mask, int32_t* out, hipStream_t s) {
    const size_t lds = walk_lds_bytes(p.cap);
    if (!lds) return 1;
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_stats<NCH>, dim3(p.G), dim3(64 * kWalkWaves), lds, s, p, mask, out));
    return 0;
}

}  // namespace ao
