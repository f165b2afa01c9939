// snapshot_check_main.cpp -- the snapshot consistency check (csrc/snapshot_check.hpp) as a stand-alone host program, for a
// sanitizer run: the check walks offsets that come from a file. No HIP, no device, nothing loaded into Python.
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/snapshot_check_main.cpp -o snapshot_check_main
//     ./snapshot_check_main
//
// Builds the two-game snapshot of tests/test_tree_snapshot_host.py in exactly-sized heap arrays (so a read past an array is
// a sanitizer report), checks that it passes, then applies one mutation per rule and checks that each is refused with a
// message naming the field. Exit status 0: everything as expected.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../alpha_omok_amd/csrc/snapshot_check.hpp"

namespace {

struct Snap {
    std::vector<int32_t> hdr, moves, nchild, parent, pedge, n, child;
    std::vector<double> gauss, p;
    std::vector<uint32_t> mt;
    std::vector<uint8_t> act;
    std::vector<float> w, q;
    ao_tree_snapshot view() {
        ao_tree_snapshot s{};
        s.board = 3; s.inplanes = 5; s.win_mark = 3; s.sims = 10; s.noise = 1; s.c_puct = 5.0;
        s.games = static_cast<int32_t>(hdr.size() / AO_SNAP_HDR);
        s.nodes = static_cast<int64_t>(nchild.size());
        s.edges = static_cast<int64_t>(act.size());
        s.hdr = hdr.data(); s.gauss = gauss.data(); s.mt = mt.data(); s.moves = moves.data();
        s.nchild = nchild.data(); s.parent = parent.data(); s.parent_edge = pedge.data();
        s.act = act.data(); s.n = n.data(); s.w = w.data(); s.q = q.data(); s.p = p.data(); s.child = child.data();
        return s;
    }
};

// game 0: one move played (cell 4), an expanded root with two expanded children and one terminal edge; game 1: fresh
Snap make() {
    Snap s;
    s.hdr = {3, 22, 1, AO_ROOT_EXPANDED, 0, 17, 0, 0, /**/ 0, 0, 0, AO_ROOT_FRESH, 0, 624, 1, 0};
    s.gauss = {0.0, -0.25};
    s.mt.assign(2 * 624, 12345u);
    s.moves.assign(2 * 9, 0);
    s.moves[0] = 4;
    s.nchild = {8, 7, 7};
    s.parent = {-1, 0, 0};
    s.pedge = {-1, 0, 1};
    const uint8_t a0[8] = {0, 1, 2, 3, 5, 6, 7, 8}, a1[7] = {1, 2, 3, 5, 6, 7, 8}, a2[7] = {0, 2, 3, 5, 6, 7, 8};
    s.act.insert(s.act.end(), a0, a0 + 8);
    s.act.insert(s.act.end(), a1, a1 + 7);
    s.act.insert(s.act.end(), a2, a2 + 7);
    s.n.assign(22, 0);
    s.child.assign(22, -1);
    s.w.assign(22, 0.f);
    s.q.assign(22, 0.f);
    s.p.assign(22, 0.125);
    s.n[0] = 3; s.child[0] = 1; s.w[0] = 1.5f; s.q[0] = 0.5f;
    s.n[1] = 2; s.child[1] = 2; s.w[1] = -1.f; s.q[1] = -0.5f;
    s.n[2] = 1; s.child[2] = -2; s.w[2] = 1.f; s.q[2] = 1.f;
    s.n[8] = 1; s.w[8] = 0.25f; s.q[8] = 0.25f;
    return s;
}

int failures = 0;

void expect(const char* what, const std::function<void(Snap&)>& mutate, const char* field) {
    Snap s = make();
    mutate(s);
    const ao_tree_snapshot v = s.view();
    const std::string why = ao::snapshot_check(&v);
    const bool ok = field ? (!why.empty() && why.find(field) != std::string::npos) : why.empty();
    std::printf("%-28s %s  %s\n", what, ok ? "ok  " : "FAIL", why.empty() ? "(accepted)" : why.c_str());
    if (!ok) ++failures;
}

}  // namespace

int main() {
    expect("unchanged", [](Snap&) {}, nullptr);
    expect("child points backwards", [](Snap& s) { s.child[8] = 0; }, "child");
    expect("node named by two edges", [](Snap& s) { s.child[3] = 2; s.n[3] = 1; }, "two edges");
    expect("wrong parent_edge", [](Snap& s) { s.pedge[2] = 0; }, "parent_edge");
    expect("wrong parent", [](Snap& s) { s.parent[2] = 1; }, "parent");
    expect("nchild = 0", [](Snap& s) { s.nchild[1] = 0; }, "nchild");
    expect("nchild beyond A - ply", [](Snap& s) { s.nchild[1] = 8; s.nchild[2] = 6; }, "nchild");
    expect("duplicate action", [](Snap& s) { s.act[9] = s.act[8]; }, "act");
    expect("action off the board", [](Snap& s) { s.act[21] = 9; }, "act");
    expect("NaN p", [](Snap& s) { s.p[5] = std::nan(""); }, "p:");
    expect("infinite w", [](Snap& s) { s.w[0] = INFINITY; }, "w:");
    expect("negative n", [](Snap& s) { s.n[4] = -1; }, "n:");
    expect("expanded child, n = 0", [](Snap& s) { s.n[1] = 0; }, "n:");
    expect("truncated edge arrays", [](Snap& s) { s.act.pop_back(); s.n.pop_back(); s.w.pop_back(); s.q.pop_back(); s.p.pop_back(); s.child.pop_back(); }, "edges");
    expect("truncated node arrays", [](Snap& s) { s.nchild.pop_back(); s.parent.pop_back(); s.pedge.pop_back(); }, "nodes");
    expect("child beyond the game", [](Snap& s) { s.child[3] = 3; s.n[3] = 1; }, "child");
    expect("child skips a number", [](Snap& s) { s.child[0] = 2; s.child[1] = 1; }, "child");
    expect("huge nchild", [](Snap& s) { s.nchild[0] = 0x7fffffff; }, "nchild");
    expect("huge node count", [](Snap& s) { s.hdr[0] = 0x7fffffff; }, "nodes");
    expect("negative edge count", [](Snap& s) { s.hdr[1] = -5; }, "edges");
    expect("pos = 625", [](Snap& s) { s.hdr[AO_SNAP_HDR + 5] = 625; }, "pos");
    expect("repeated root move", [](Snap& s) { s.hdr[AO_SNAP_HDR + 2] = 2; s.moves[9] = 3; s.moves[10] = 3; }, "moves");
    expect("root move off the board", [](Snap& s) { s.moves[0] = 9; }, "moves");
    expect("too many moves", [](Snap& s) { s.hdr[2] = 10; }, "moves");
    expect("tree below a fresh root", [](Snap& s) { s.hdr[3] = AO_ROOT_FRESH; }, "status");
    expect("finished game with a tree", [](Snap& s) { s.hdr[4] = 1; }, "over");
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
