// snapshot_check.hpp -- consistency of a tree snapshot (ao_tree_snapshot, include/omok_hip.h). Host code only, no HIP: the
// check walks offsets that come from a file, so it is kept where a host sanitizer can reach it (tools/snapshot_check_main.cpp
// builds it into a stand-alone program). ao_tree_import runs it before anything is uploaded: what passes here lets
// k_tree_unpack (tree_snapshot.hip) read only inside the uploaded arrays and write only inside the game's arena.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/omok_hip.h"

namespace ao {

constexpr int kSnapMaxBoard = 15;   // engine_types.hpp kMaxBoard (not included here: that header pulls in the HIP runtime)

// Empty string: the snapshot is consistent. Otherwise the first violation, naming the field.
inline std::string snapshot_check(const ao_tree_snapshot* s) {
    if (!s) return "null snapshot";
    if (s->board < 3 || s->board > kSnapMaxBoard) return "board: must be in 3..15";
    if (s->games < 0) return "games: negative";
    if (s->nodes < 0 || s->edges < 0) return "nodes / edges: negative array length";
    const int A = s->board * s->board;
    if (s->games > 0 && (!s->hdr || !s->gauss || !s->mt || !s->moves)) return "hdr / gauss / mt / moves: null array";
    if (s->nodes > 0 && (!s->nchild || !s->parent || !s->parent_edge)) return "nchild / parent / parent_edge: null array";
    if (s->edges > 0 && (!s->act || !s->n || !s->w || !s->q || !s->p || !s->child)) return "act / n / w / q / p / child: null array";
    auto at = [](int game, const std::string& m) { return "game " + std::to_string(game) + ": " + m; };
    // sizes first: nothing below reads an array before these sums have placed every game inside it
    int64_t nsum = 0, esum = 0;
    for (int i = 0; i < s->games; ++i) {
        const int32_t* h = s->hdr + static_cast<size_t>(i) * AO_SNAP_HDR;
        if (h[0] < 0) return at(i, "nodes: negative");
        if (h[1] < 0) return at(i, "edges: negative");
        if (h[0] == 0 && h[1] != 0) return at(i, "edges: a game without nodes has edges");
        nsum += h[0];
        esum += h[1];
        if (nsum > s->nodes) return at(i, "nodes: the games' node counts exceed the node arrays (" + std::to_string(s->nodes) + ")");
        if (esum > s->edges) return at(i, "edges: the games' edge counts exceed the edge arrays (" + std::to_string(s->edges) + ")");
    }
    if (nsum != s->nodes) return "nodes: the node arrays hold " + std::to_string(s->nodes) + " entries, the games' counts sum to " + std::to_string(nsum);
    if (esum != s->edges) return "edges: the edge arrays hold " + std::to_string(s->edges) + " entries, the games' counts sum to " + std::to_string(esum);

    int64_t nb = 0, eb = 0;   // first node / edge of the game
    std::vector<int32_t> ply, first;
    std::vector<uint8_t> named;
    for (int i = 0; i < s->games; ++i) {
        const int32_t* h = s->hdr + static_cast<size_t>(i) * AO_SNAP_HDR;
        const int nodes = h[0], edges = h[1], nmoves = h[2], status = h[3], over = h[4], pos = h[5], has_gauss = h[6];
        if (nmoves < 0 || nmoves > A) return at(i, "moves: the count must be in 0..A");
        {
            uint8_t used[kSnapMaxBoard * kSnapMaxBoard] = {};
            const int32_t* mv = s->moves + static_cast<size_t>(i) * A;
            for (int k = 0; k < nmoves; ++k) {
                if (mv[k] < 0 || mv[k] >= A) return at(i, "moves: move " + std::to_string(k) + " is off the board");
                if (used[mv[k]]) return at(i, "moves: cell " + std::to_string(mv[k]) + " is played twice");
                used[mv[k]] = 1;
            }
        }
        if (status < AO_ROOT_FRESH || status > AO_ROOT_EXPANDED) return at(i, "status: not an AO_ROOT_* value");
        if (over < 0 || over > 3) return at(i, "over: not a win index");
        if ((status == AO_ROOT_EXPANDED) != (nodes > 0)) return at(i, "status: an expanded root and no nodes, or nodes below a root that is not expanded");
        if (over != 0 && nodes > 0) return at(i, "over: a finished game keeps no tree");
        if (pos < 0 || pos > 624) return at(i, "pos: must be in 0..624");
        if (has_gauss != 0 && has_gauss != 1) return at(i, "has_gauss: must be 0 or 1");
        if (!std::isfinite(s->gauss[i])) return at(i, "gauss: not finite");
        if (nodes == 0) continue;

        const int32_t* nchild = s->nchild + nb;
        const int32_t* parent = s->parent + nb;
        const int32_t* pedge = s->parent_edge + nb;
        first.assign(static_cast<size_t>(nodes), 0);
        int64_t run = 0;
        for (int k = 0; k < nodes; ++k) {
            if (nchild[k] < 1 || nchild[k] > A) return at(i, "nchild: node " + std::to_string(k) + " has " + std::to_string(nchild[k]) + " edges (1..A)");
            first[k] = static_cast<int32_t>(run);
            run += nchild[k];
            if (run > edges) return at(i, "nchild: the running sum passes the game's " + std::to_string(edges) + " edges at node " + std::to_string(k));
        }
        if (run != edges) return at(i, "nchild: the sum " + std::to_string(run) + " is not the game's " + std::to_string(edges) + " edges");
        if (parent[0] != -1 || pedge[0] != -1) return at(i, "parent / parent_edge: the root (node 0) must have -1");

        ply.assign(static_cast<size_t>(nodes), 0);
        named.assign(static_cast<size_t>(nodes), 0);
        ply[0] = nmoves;
        named[0] = 1;
        int next = 1;   // the node number the next expanded child must carry
        for (int k = 0; k < nodes; ++k) {
            const std::string nk = "node " + std::to_string(k);
            if (!named[k]) return at(i, "child: " + nk + " is named by no edge");
            if (nchild[k] > A - ply[k]) return at(i, "nchild: " + nk + " at ply " + std::to_string(ply[k]) + " has " + std::to_string(nchild[k]) + " edges, more than A - ply");
            uint8_t used[kSnapMaxBoard * kSnapMaxBoard] = {};
            for (int j = 0; j < nchild[k]; ++j) {
                const int64_t e = eb + first[k] + j;
                const std::string ne = nk + " edge " + std::to_string(j);
                const int a = s->act[e];
                if (a >= A) return at(i, "act: " + ne + " is off the board");
                if (used[a]) return at(i, "act: " + ne + " repeats action " + std::to_string(a) + " of its node");
                used[a] = 1;
                const int32_t ch = s->child[e];
                if (s->n[e] < 0) return at(i, "n: " + ne + " is negative");
                if (!std::isfinite(s->w[e])) return at(i, "w: " + ne + " is not finite");
                if (!std::isfinite(s->q[e])) return at(i, "q: " + ne + " is not finite");
                if (!std::isfinite(s->p[e])) return at(i, "p: " + ne + " is not finite");
                if (ch < -2) return at(i, "child: " + ne + " is neither a node number nor -1 / -2");
                if (ch != -1 && s->n[e] < 1) return at(i, "n: " + ne + " has an expanded or terminal child and no visit");
                if (ch < 0) continue;
                if (ch <= k) return at(i, "child: " + ne + " points backwards, to node " + std::to_string(ch));
                if (ch >= nodes) return at(i, "child: " + ne + " names node " + std::to_string(ch) + " of " + std::to_string(nodes));
                if (named[ch]) return at(i, "child: node " + std::to_string(ch) + " is named by two edges");
                if (ch != next) return at(i, "child: " + ne + " names node " + std::to_string(ch) + " where scan order (breadth first) has " + std::to_string(next));
                if (parent[ch] != k) return at(i, "parent: node " + std::to_string(ch) + " says " + std::to_string(parent[ch]) + ", the edge naming it belongs to node " + std::to_string(k));
                if (pedge[ch] != j) return at(i, "parent_edge: node " + std::to_string(ch) + " says " + std::to_string(pedge[ch]) + ", the edge naming it is edge " + std::to_string(j));
                named[ch] = 1;
                ply[ch] = ply[k] + 1;
                ++next;
            }
        }
        nb += nodes;
        eb += edges;
    }
    return std::string();
}

}  // namespace ao
