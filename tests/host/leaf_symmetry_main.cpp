// Stand-alone host program over alpha_omok_amd/csrc/symmetry.hpp (tests/test_leaf_symmetry_host.py). One query per line of
// stdin, one answer per line of stdout:
//   cell s c B        ->  sym_cell sym_cell_inv sym_inverse
//   leaf key ply sim  ->  leaf_symmetry
//   key base seed     ->  leaf_key
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "symmetry.hpp"

int main() {
    char what[16];
    unsigned long long a, b, c;
    while (std::scanf("%15s %llu %llu", what, &a, &b) == 3) {
        if (!std::strcmp(what, "key")) {
            std::printf("%u\n", ao::leaf_key(static_cast<uint32_t>(a), static_cast<uint32_t>(b)));
            continue;
        }
        if (std::scanf("%llu", &c) != 1) return 2;
        if (!std::strcmp(what, "cell")) {
            const int s = static_cast<int>(a), cell = static_cast<int>(b), B = static_cast<int>(c);
            std::printf("%d %d %d\n", ao::sym_cell(s, cell, B), ao::sym_cell_inv(s, cell, B), ao::sym_inverse(s));
        } else if (!std::strcmp(what, "leaf")) {
            std::printf("%d\n", ao::leaf_symmetry(static_cast<uint32_t>(a), static_cast<uint32_t>(b), static_cast<uint32_t>(c)));
        } else {
            return 3;
        }
    }
    return 0;
}
