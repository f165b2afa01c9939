// replay_snapshot_check_main.cpp -- the replay snapshot's canonical-form check (csrc/replay_snapshot_check.hpp) as a
// stand-alone host program, for a sanitizer run: the check walks lengths that come from a file. No HIP, no device, nothing
// loaded into Python.
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/replay_snapshot_check_main.cpp -o replay_snapshot_check_main
//     ./replay_snapshot_check_main
//
// Builds the four-entry snapshot of tests/test_replay_snapshot_host.py in exactly-sized heap arrays (so a read past an array
// is a sanitizer report), checks that it passes, then applies one mutation per rule and checks that each is refused with a
// message naming the field. The same on a 9x9 snapshot, whose last word holds 17 valid bits. Exit status 0: everything as
// expected.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "../alpha_omok_amd/csrc/replay_snapshot_check.hpp"

namespace {

struct Snap {
    int board = 3, inplanes = 2, format = 1, words = 1;
    std::vector<uint8_t> kind;
    std::vector<float> z, raw;
    std::vector<uint64_t> bits, mask;
    std::vector<double> val;
    static constexpr int64_t kAuto = std::numeric_limits<int64_t>::min();
    int64_t entries = kAuto, pi_values = kAuto, raw_entries = kAuto;   // kAuto: derived from the arrays
    ao_replay_snapshot view() {
        ao_replay_snapshot s{};
        s.board = board; s.inplanes = inplanes; s.format = format; s.words = words;
        s.entries = entries != kAuto ? entries : static_cast<int64_t>(kind.size());
        s.pi_values = pi_values != kAuto ? pi_values : static_cast<int64_t>(val.size());
        s.raw_entries = raw_entries != kAuto ? raw_entries : static_cast<int64_t>(raw.size() / (static_cast<size_t>(inplanes) * board * board));
        s.kind = kind.data(); s.z = z.data(); s.bits = bits.data(); s.pi_mask = mask.data(); s.pi_val = val.data(); s.raw = raw.data();
        return s;
    }
};

// 3x3, two planes. Entry 0: one-hot pi; entry 1: dense pi with -0.0, a NaN and a subnormal; entry 2: kind 1 (raw planes), pi
// over three cells; entry 3: all-zero pi.
Snap make3() {
    Snap s;
    s.kind = {0, 0, 1, 0};
    s.z = {1.f, -1.f, 0.f, 1.f};
    s.bits = {0x011, 0x1ff, 0x0a2, 0x000, 0, 0, 0x100, 0x0ff};
    s.mask = {0x010, 0x1ff, 0x007, 0x000};
    s.val = {1.0};
    const double dense[9] = {0.125, -0.0, std::numeric_limits<double>::quiet_NaN(), 4.9406564584124654e-324, 0.25, 0.125, 0.125, 0.125, 0.25};
    s.val.insert(s.val.end(), dense, dense + 9);
    s.val.insert(s.val.end(), {0.5, 0.25, 0.25});
    s.raw.assign(2 * 9, 0.f);
    s.raw[0] = 0.5f; s.raw[4] = 2.f; s.raw[9] = -0.f; s.raw[17] = 1.f;
    return s;
}

// 9x9 (W = 2, 17 valid bits in the last word), one plane, two entries
Snap make9() {
    Snap s;
    s.board = 9; s.inplanes = 1; s.words = 2;
    s.kind = {0, 0};
    s.z = {1.f, -1.f};
    s.bits = {~0ull, 0x1ffffull, 1ull, 0x10000ull};
    s.mask = {0ull, 0x10000ull, ~0ull, 0x1ffffull};
    s.val.assign(1 + 81, 1.0 / 81);
    return s;
}

int failures = 0;

void expect(const char* what, Snap (*make)(), const std::function<void(Snap&)>& mutate, const char* field) {
    Snap s = make();
    mutate(s);
    const ao_replay_snapshot v = s.view();
    const std::string why = ao::replay_snapshot_check(&v);
    const bool ok = field ? (!why.empty() && why.find(field) != std::string::npos) : why.empty();
    std::printf("%-34s %s  %s\n", what, ok ? "ok  " : "FAIL", why.empty() ? "(accepted)" : why.c_str());
    if (!ok) ++failures;
}

}  // namespace

int main() {
    expect("3x3 unchanged", make3, [](Snap&) {}, nullptr);
    expect("9x9 unchanged", make9, [](Snap&) {}, nullptr);
    expect("empty snapshot", make3, [](Snap& s) { s = Snap(); }, nullptr);
    expect("board 2", make3, [](Snap& s) { s.board = 2; }, "board");
    expect("board 16", make3, [](Snap& s) { s.board = 16; }, "board");
    expect("inplanes 0", make3, [](Snap& s) { s.inplanes = 0; s.raw_entries = 1; }, "inplanes");
    expect("inplanes 33", make3, [](Snap& s) { s.inplanes = 33; s.raw_entries = 1; }, "inplanes");
    expect("format 2", make3, [](Snap& s) { s.format = 2; }, "format");
    expect("words 2 on a 3x3 board", make3, [](Snap& s) { s.words = 2; }, "words");
    expect("words 1 on a 9x9 board", make9, [](Snap& s) { s.words = 1; }, "words");
    expect("mask bit at cell A", make3, [](Snap& s) { s.mask[3] = 1ull << 9; s.val.push_back(1.0); }, "pi_mask");
    expect("mask bit 63", make3, [](Snap& s) { s.mask[0] |= 1ull << 63; s.val.push_back(1.0); }, "pi_mask");
    expect("9x9 mask bit at cell 81", make9, [](Snap& s) { s.mask[1] |= 1ull << 17; s.val.push_back(1.0); }, "pi_mask");
    expect("plane bit at cell A", make3, [](Snap& s) { s.bits[1] |= 1ull << 9; }, "bits");
    expect("9x9 plane bit at cell 81", make9, [](Snap& s) { s.bits[3] |= 1ull << 17; }, "bits");
    expect("kind 2", make3, [](Snap& s) { s.kind[1] = 2; }, "kind");
    expect("bits on a kind-1 row", make3, [](Snap& s) { s.bits[5] = 1; }, "bits");
    expect("pi_values one short", make3, [](Snap& s) { s.val.pop_back(); }, "pi_values");
    expect("pi_values one long", make3, [](Snap& s) { s.val.push_back(1.0); }, "pi_values");
    expect("huge mask sum, short pi_val", make3, [](Snap& s) { s.mask[0] = 0x1ff; }, "pi_values");
    expect("raw_entries one short", make3, [](Snap& s) { s.raw.clear(); }, "raw_entries");
    expect("raw_entries one long", make3, [](Snap& s) { s.raw.resize(2 * 2 * 9); }, "raw_entries");
    expect("kind flipped to 0", make3, [](Snap& s) { s.kind[2] = 0; }, "raw_entries");
    expect("zero pattern in pi_val", make3, [](Snap& s) { s.val[4] = 0.0; }, "pi_val");
    expect("negative entries", make3, [](Snap& s) { s.entries = -1; }, "entries");
    expect("negative pi_values", make3, [](Snap& s) { s.pi_values = -1; }, "pi_values");
    expect("negative raw_entries", make3, [](Snap& s) { s.raw_entries = -1; }, "raw_entries");
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
