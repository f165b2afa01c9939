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
//
// The host side of the three calls (ao_tree_lookup, ao_tree_pv, ao_tree_stats) follows the kernels: each lays out the engine's
// read-out workspace right above the launch that reads it.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
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
// launchers
// ----------------------------------------------------------------------------------------------

static void launch_tree_lookup(const TreeParams& p, const int32_t* queries, int n, int stride, const LookupOut& o, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((n + kReadPerWG - 1) / kReadPerWG)), block(64 * kReadPerWG);
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_lookup<NCH>, grid, block, 0, s, p, queries, n, stride, o));
}

static void launch_tree_pv(const TreeParams& p, const uint8_t* mask, int max_len, int32_t* act, int32_t* n, float* q, int32_t* len, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((p.G + kReadPerWG - 1) / kReadPerWG)), block(64 * kReadPerWG);
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_pv<NCH>, grid, block, 0, s, p, mask, max_len, act, n, q, len));
}

// non-zero: the queue of a `cap`-node arena does not fit the LDS of one workgroup (walk_lds_bytes) -- nothing is launched
static int launch_tree_stats(const TreeParams& p, const uint8_t* mask, int32_t* out, hipStream_t s) {
    const size_t lds = walk_lds_bytes(p.cap);
    if (!lds) return 1;
    AO_DISPATCH_NCH(nch_of_cells(p.A), hipLaunchKernelGGL(k_tree_stats<NCH>, dim3(p.G), dim3(64 * kWalkWaves), lds, s, p, mask, out));
    return 0;
}

// ----------------------------------------------------------------------------------------------
// the host side: one device workspace of the engine (d_ro, grown on demand) and its host mirror (h_ro), shared with the other
// calls that read trees or roots in bulk (tree_proofs.hip, root_tactics.hip, tree_snapshot.hip)
// ----------------------------------------------------------------------------------------------
int readout_begin(ao_engine* e, const char* who, size_t bytes) {
    if (e->in_move) return e->fail(std::string(who) + " inside a move (between ao_begin_move and ao_end_move)");
    AO_HIP(e, hipSetDevice(e->cfg.device));
    if (bytes > e->d_ro.n) {
        AO_HIP(e, hipStreamSynchronize(e->stream));   // nothing queued reads the old workspace
        if (e->d_ro.reserve(e, bytes)) return 1;
    }
    if (e->h_ro.size() < bytes) e->h_ro.resize(bytes);
    return 0;
}

// per game: 0 = not asked for, 1 = asked for, 2 = asked for and the root is a key of the reference's dict
void readout_mask(const ao_engine* e, const uint8_t* mask, uint8_t* out) {
    for (int g = 0; g < e->G; ++g)
        out[g] = (mask && !mask[g]) ? 0 : (e->status[g] != AO_ROOT_FRESH ? 2 : 1);
}

}  // namespace ao

extern "C" {

// replaces self.tree[node_id] (agents.py:52,206-210)
int ao_tree_lookup(ao_engine* e, const int32_t* games, const int32_t* moves, int32_t stride, const int32_t* m, int32_t n,
                   int32_t* status, double* node_nwqp, int32_t* nchild, int32_t* child_action, int32_t* child_n, float* child_w,
                   float* child_q, double* child_p) {
    constexpr int kChunk = 1024;   // queries per launch
    if (e->in_move) return e->fail("ao_tree_lookup inside a move (between ao_begin_move and ao_end_move)");
    if (n < 0 || stride < 0) return e->fail("ao_tree_lookup: negative query count or stride");
    if (n == 0) return 0;
    if (!games || !m || (!moves && stride > 0)) return e->fail("ao_tree_lookup: null argument");
    const int A = e->A;
    for (int i = 0; i < n; ++i) {
        if (games[i] < 0 || games[i] >= e->G) return e->fail("game index out of range");
        if (m[i] < 0) return e->fail("ao_tree_lookup: negative id length");
        if (m[i] > stride && m[i] <= A) return e->fail("ao_tree_lookup: m[i] exceeds the row stride");
    }
    const bool kids = child_action || child_n || child_w || child_q || child_p;
    const size_t qs = 3 + static_cast<size_t>(A);   // a query row: game, suffix length, root_known, suffix
    const size_t in_bytes = kChunk * qs * 4;
    const size_t out_bytes = static_cast<size_t>(kChunk) * (32 + 8 + (kids ? 24 * static_cast<size_t>(A) : 0));
    if (readout_begin(e, "ao_tree_lookup", in_bytes + out_bytes)) return 1;
    for (int64_t first = 0; first < n; first += kChunk) {
        const int c = static_cast<int>(std::min<int64_t>(kChunk, n - first));
        const size_t cA = static_cast<size_t>(c) * A;
        int32_t* hq = reinterpret_cast<int32_t*>(e->h_ro.data());
        for (int k = 0; k < c; ++k) {
            const int64_t i = first + k;
            const int g = games[i];
            const std::vector<int32_t>& cur = e->moves[g];
            const int32_t* id = moves + i * static_cast<int64_t>(stride);
            int32_t* row = hq + static_cast<size_t>(k) * qs;
            const bool extends = m[i] <= A && static_cast<size_t>(m[i]) >= cur.size() && std::equal(cur.begin(), cur.end(), id);
            row[0] = g;
            row[1] = extends ? m[i] - static_cast<int>(cur.size()) : -1;
            row[2] = e->status[g] != AO_ROOT_FRESH ? 1 : 0;
            if (extends) std::copy(id + cur.size(), id + m[i], row + 3);
        }
        // device layout of a chunk of c queries: the 8-byte arrays first
        unsigned char* d = e->d_ro.p + in_bytes;
        double* d_nwqp = reinterpret_cast<double*>(d);
        double* d_cp = d_nwqp + 4 * static_cast<size_t>(c);
        int32_t* d_status = reinterpret_cast<int32_t*>(d_cp + (kids ? cA : 0));
        int32_t* d_nchild = d_status + c;
        int32_t* d_ca = d_nchild + c;
        int32_t* d_cn = d_ca + cA;
        float* d_cw = reinterpret_cast<float*>(d_cn + cA);
        float* d_cq = d_cw + cA;
        const size_t used = static_cast<size_t>(c) * (32 + 8 + (kids ? 24 * static_cast<size_t>(A) : 0));
        AO_HIP(e, hipMemcpyAsync(e->d_ro.p, hq, static_cast<size_t>(c) * qs * 4, hipMemcpyHostToDevice, e->stream));
        const ao::LookupOut o{d_status, d_nchild, d_nwqp, kids ? d_ca : nullptr, kids ? d_cn : nullptr, kids ? d_cw : nullptr,
                              kids ? d_cq : nullptr, kids ? d_cp : nullptr};
        ao::launch_tree_lookup(e->tp, reinterpret_cast<const int32_t*>(e->d_ro.p), c, static_cast<int>(qs), o, e->stream);
        AO_HIP(e, hipGetLastError());
        unsigned char* h = e->h_ro.data() + in_bytes;
        AO_HIP(e, hipMemcpyAsync(h, d, used, hipMemcpyDeviceToHost, e->stream));
        AO_HIP(e, hipStreamSynchronize(e->stream));   // the staging buffers are reused by the next chunk
        auto at = [&](const void* dev) { return h + (static_cast<const unsigned char*>(dev) - d); };
        if (node_nwqp) std::memcpy(node_nwqp + 4 * first, at(d_nwqp), sizeof(double) * 4 * c);
        if (status) std::memcpy(status + first, at(d_status), sizeof(int32_t) * c);
        if (nchild) std::memcpy(nchild + first, at(d_nchild), sizeof(int32_t) * c);
        if (child_action) std::memcpy(child_action + first * A, at(d_ca), sizeof(int32_t) * cA);
        if (child_n) std::memcpy(child_n + first * A, at(d_cn), sizeof(int32_t) * cA);
        if (child_w) std::memcpy(child_w + first * A, at(d_cw), sizeof(float) * cA);
        if (child_q) std::memcpy(child_q + first * A, at(d_cq), sizeof(float) * cA);
        if (child_p) std::memcpy(child_p + first * A, at(d_cp), sizeof(double) * cA);
    }
    return 0;
}

// the line the search expects to be played: arg-max of agents.py:67-69's visit vector, node after node
int ao_tree_pv(ao_engine* e, const uint8_t* mask, int32_t max_len, int32_t* action, int32_t* n, float* q, int32_t* len) {
    if (e->in_move) return e->fail("ao_tree_pv inside a move (between ao_begin_move and ao_end_move)");
    if (max_len < 1 || max_len > e->A) return e->fail("ao_tree_pv: max_len must be in 1..A");
    const size_t G = static_cast<size_t>(e->G), GL = G * static_cast<size_t>(max_len);
    const size_t out_bytes = (3 * GL + G) * 4;
    if (readout_begin(e, "ao_tree_pv", out_bytes + G)) return 1;
    uint8_t* h_mask = e->h_ro.data() + out_bytes;
    readout_mask(e, mask, h_mask);
    uint8_t* d_mask = e->d_ro.p + out_bytes;
    int32_t* d_act = reinterpret_cast<int32_t*>(e->d_ro.p);
    int32_t* d_n = d_act + GL;
    float* d_q = reinterpret_cast<float*>(d_n + GL);
    int32_t* d_len = reinterpret_cast<int32_t*>(d_q + GL);
    AO_HIP(e, hipMemcpyAsync(d_mask, h_mask, G, hipMemcpyHostToDevice, e->stream));
    ao::launch_tree_pv(e->tp, d_mask, max_len, d_act, d_n, d_q, d_len, e->stream);
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipMemcpyAsync(e->h_ro.data(), e->d_ro.p, out_bytes, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    const int32_t* h_act = reinterpret_cast<const int32_t*>(e->h_ro.data());
    const int32_t* h_n = h_act + GL;
    const float* h_q = reinterpret_cast<const float*>(h_n + GL);
    const int32_t* h_len = reinterpret_cast<const int32_t*>(h_q + GL);
    for (size_t g = 0; g < G; ++g) {
        if (!h_mask[g]) continue;
        const size_t l = static_cast<size_t>(h_len[g]), o = g * max_len;
        if (action) std::memcpy(action + o, h_act + o, 4 * l);
        if (n) std::memcpy(n + o, h_n + o, 4 * l);
        if (q) std::memcpy(q + o, h_q + o, 4 * l);
        if (len) len[g] = h_len[g];
    }
    return 0;
}

// replaces the prints of del_parents (agents.py:241-250)
int ao_tree_stats(ao_engine* e, const uint8_t* mask, int32_t* out) {
    if (e->in_move) return e->fail("ao_tree_stats inside a move (between ao_begin_move and ao_end_move)");
    if (!out) return e->fail("ao_tree_stats: null output");
    const size_t G = static_cast<size_t>(e->G);
    if (readout_begin(e, "ao_tree_stats", 16 * G + G)) return 1;
    uint8_t* h_mask = e->h_ro.data() + 16 * G;
    readout_mask(e, mask, h_mask);
    uint8_t* d_mask = e->d_ro.p + 16 * G;
    AO_HIP(e, hipMemcpyAsync(d_mask, h_mask, G, hipMemcpyHostToDevice, e->stream));
    if (ao::launch_tree_stats(e->tp, d_mask, reinterpret_cast<int32_t*>(e->d_ro.p), e->stream))
        return queue_refused(e, "ao_tree_stats");
    AO_HIP(e, hipGetLastError());
    AO_HIP(e, hipMemcpyAsync(e->h_ro.data(), e->d_ro.p, 16 * G, hipMemcpyDeviceToHost, e->stream));
    AO_HIP(e, hipStreamSynchronize(e->stream));
    const int32_t* h = reinterpret_cast<const int32_t*>(e->h_ro.data());
    for (size_t g = 0; g < G; ++g)
        if (h_mask[g] && h[4 * g] < 0) return e->fail("ao_tree_stats: game " + std::to_string(g) + ": the tree reaches more nodes than the arena holds (inconsistent tree)");
    for (size_t g = 0; g < G; ++g)
        if (h_mask[g]) std::memcpy(out + 4 * g, h + 4 * g, 16);
    return 0;
}

}  // extern "C"
