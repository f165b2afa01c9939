// symmetry.hpp -- the eight symmetries of the square board, as index maps, for host and device.
//
// Numbering: s = 2*r + f -- rot90 (counter-clockwise, np.rot90) by r, then a flip of the last axis if f. It is the order of
// utils.augment_dataset and of the replay ring ([r0, r0 flipped, r1, r1 flipped, ...]); s = 0 is the identity.
// alpha_omok_amd/utils.py holds the same functions (sym_cell, sym_inverse, leaf_symmetry, leaf_key); the two agree bit for
// bit (tests/test_leaf_symmetry_host.py compiles this header into a host program and compares).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AO_SYM_FN __host__ __device__ inline
#else
#define AO_SYM_FN inline
#endif

namespace ao {

// source cell of output cell (i, j) under symmetry sym: X'[i][j] = X[source]
AO_SYM_FN int sym_source(int sym, int i, int j, int B) {
    const int r = sym >> 1;
    const int jj = (sym & 1) ? B - 1 - j : j;
    int si, sj;
    switch (r) {
        case 0: si = i; sj = jj; break;
        case 1: si = jj; sj = B - 1 - i; break;
        case 2: si = B - 1 - i; sj = B - 1 - jj; break;
        default: si = B - 1 - jj; sj = i; break;
    }
    return si * B + sj;
}

// sym_planes(X, s)[..., c] = X[..., sym_cell(s, c, B)]
AO_SYM_FN int sym_cell(int sym, int c, int B) {
    const int i = c / B;
    return sym_source(sym, i, c - i * B, B);
}

// The symmetry that undoes s: a rotation is undone by the opposite rotation, a rotation followed by a flip is a reflection
// and undoes itself. sym_cell(sym_inverse(s), sym_cell(s, c)) == c.
AO_SYM_FN int sym_inverse(int sym) { return (sym & 1) ? sym : ((8 - sym) & 7); }

// where source cell d goes: the output cell c with sym_cell(s, c) == d
AO_SYM_FN int sym_cell_inv(int sym, int d, int B) { return sym_cell(sym_inverse(sym), d, B); }

// The symmetry a leaf is evaluated under: a stateless function of the game's key, the number of stones on the leaf's board
// and the game's 0-based simulation index inside the current move (arithmetic mod 2^32).
AO_SYM_FN int leaf_symmetry(uint32_t key, uint32_t ply, uint32_t sim) {
    uint32_t x = key ^ (ply * 0x9E3779B1u) ^ (sim * 0x85EBCA77u);
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return static_cast<int>(x >> 29);
}

// the key of a game from the caller's base key and the game's seed
AO_SYM_FN uint32_t leaf_key(uint32_t base, uint32_t seed) { return base ^ (seed * 0xC2B2AE35u); }

}  // namespace ao
