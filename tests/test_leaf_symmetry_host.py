"""The definitions behind leaf symmetries, on the host: alpha_omok_amd/csrc/symmetry.hpp -- compiled into a stand-alone program
(tests/host/leaf_symmetry_main.cpp) with the host C++ compiler -- against alpha_omok_amd/utils.py, and utils against
augment_dataset, which is where the numbering s = 2*r + f comes from. No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

from alpha_omok_amd import utils

CSRC = os.path.join(REPO, "alpha_omok_amd", "csrc")
MAIN = os.path.join(REPO, "tests", "host", "leaf_symmetry_main.cpp")
BOARDS = (3, 4, 9, 15)
STUB_MODE = 0   # the stub the GPU tests drive the engine with (tests/test_gpu_leaf_symmetry.py imports it)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("leaf_symmetry") / "leaf_symmetry")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, MAIN, "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def test_header_cells_agree_with_utils(program):
    q = [(s, c, B) for B in BOARDS for s in range(8) for c in range(B * B)]
    out = program(["cell %d %d %d" % t for t in q])
    for (s, c, B), line in zip(q, out):
        cell, inv, sinv = map(int, line.split())
        assert cell == utils.sym_cell(s, c, B), (s, c, B)
        assert inv == utils.sym_cell_inv(s, c, B), (s, c, B)
        assert sinv == utils.sym_inverse(s)
        assert utils.sym_cell(s, inv, B) == c and utils.sym_cell_inv(s, cell, B) == c   # inverse on both sides


def test_header_leaf_symmetry_and_key_agree_with_utils(program):
    rng = np.random.RandomState(5)
    keys = [0, 1, 0xFFFFFFFF, 0x80000000] + [int(k) for k in rng.randint(0, 2 ** 32, size=60, dtype=np.uint64)]
    q = [(k, int(rng.randint(0, 226)), int(rng.randint(0, 1700))) for k in keys for _ in range(50)]
    q += [(0xFFFFFFFF, 225, 0xFFFFFFFF), (0, 0, 0)]
    out = program(["leaf %d %d %d" % t for t in q])
    assert len(q) > 3000
    for t, line in zip(q, out):
        assert int(line) == utils.leaf_symmetry(*t), t
        assert 0 <= int(line) < 8
    kq = [(int(a), int(b)) for a, b in rng.randint(0, 2 ** 32, size=(200, 2), dtype=np.uint64)] + [(0, 0), (7, 0), (0xFFFFFFFF, 0xFFFFFFFF)]
    for (a, b), line in zip(kq, program(["key %d %d" % t for t in kq])):
        assert int(line) == utils.leaf_key(a, b)
    assert utils.leaf_key(7, 0) == 7   # a ZeroAgent's single game is never seeded: its key is the base key


def test_leaf_symmetry_by_hand():
    """The finaliser worked out step by step for one input, independent of utils' loop."""
    key, ply, sim = 0x12345678, 3, 5
    M = 0xFFFFFFFF
    x = key ^ ((ply * 0x9E3779B1) & M) ^ ((sim * 0x85EBCA77) & M)
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M
    x = x ^ (x >> 16)
    assert utils.leaf_symmetry(key, ply, sim) == x >> 29


@pytest.mark.parametrize("B", BOARDS)
def test_sym_planes_is_augment_dataset(B):
    rng = np.random.RandomState(B)
    x = rng.rand(5, B, B)
    pi = rng.rand(B * B)
    aug = utils.augment_dataset([(x, pi, 1.0)], B)
    assert len(aug) == 8
    for s in range(8):
        assert np.array_equal(utils.sym_planes(x, s), aug[s][0]), s
        assert np.array_equal(utils.sym_planes(pi, s, B), aug[s][1]), s
        assert np.array_equal(utils.sym_policy_back(utils.sym_planes(pi, s, B), s), pi), s
        assert np.array_equal(utils.sym_planes(utils.sym_policy_back(pi, s), s, B), pi), s
    assert np.array_equal(utils.sym_planes(x, 0), x)


def test_every_symmetry_occurs_within_a_move():
    """Over 4096 consecutive simulation indices each of the eight symmetries occurs, for a spread of keys and plies: the
    constants do not leave the top three bits stuck."""
    rng = np.random.RandomState(9)
    for key in [0, 1, 0xFFFFFFFF] + [int(k) for k in rng.randint(0, 2 ** 32, size=8, dtype=np.uint64)]:
        for ply in (0, 1, 17, 224):
            cnt = np.bincount([utils.leaf_symmetry(key, ply, sim) for sim in range(4096)], minlength=8)
            assert cnt.min() > 0, (key, ply, cnt)
            assert cnt.min() > 512 - 6 * 22 and cnt.max() < 512 + 6 * 22, (key, ply, cnt)   # binomial(4096, 1/8): sigma = 21.2


def test_stub_evaluator_is_not_blind_to_symmetries(oracle):
    """The GPU tests tell a symmetric search from a plain one only if the evaluator is not equivariant: stub_eval of the
    transformed planes must differ from the transformed stub_eval, for every s != 0, on a sample of positions."""
    rng = np.random.RandomState(3)
    for B in (4, 9, 15):
        for _ in range(6):
            k = int(rng.randint(0, B * B // 2))
            mv = [int(m) for m in rng.permutation(B * B)[:k]]
            x = oracle.get_state_pt(mv, B, 5)
            p, _ = oracle.stub_eval(x, STUB_MODE)
            for s in range(1, 8):
                p2, _ = oracle.stub_eval(utils.sym_planes(x, s), STUB_MODE)
                assert not np.array_equal(utils.sym_policy_back(p2, s), p), (B, mv, s)
