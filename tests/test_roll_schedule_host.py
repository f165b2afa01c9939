"""The host rules of the rolling search: alpha_omok_amd/csrc/roll_schedule.hpp, compiled into a stand-alone program
(tests/host/roll_schedule_main.cpp) with the host C++ compiler and fed cases on stdin. What it prints is compared with the same
rules written out below in Python -- restated from the text of the feature (tau = ply < tau_plies; the budget and the noise
switch are column min(ply, stride - 1) of the game's table row; a fresh root runs one simulation more; a game turns when it is in
a move, has done == target and no leaf under way; a draining roll begins no move; a run returns on a record, on an empty roll or
on its launch bound; per period turn_every - 1 launches, the look, one launch, the turn), not from the header -- and with cases
worked out by hand. Also here: the Python and C entry points of the roll exist."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "alpha_omok_amd", "csrc")
MAIN = os.path.join(REPO, "tests", "host", "roll_schedule_main.cpp")
FRESH, KNOWN, EXPANDED = 0, 1, 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("roll_schedule") / "roll_schedule")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, MAIN, "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------
def next_move(ply, tau_plies, engine_noise, S, status, sims, noise):
    """sims / noise: the game's table rows (lists) or None; tau_plies None: tau 1 always."""
    tau = 1 if tau_plies is None or ply < tau_plies else 0
    budget = S if sims is None else sims[min(ply, len(sims) - 1)]
    wants = engine_noise if noise is None else bool(noise[min(ply, len(noise) - 1)])
    refuse = 1 if not 1 <= budget <= S else (2 if wants and not engine_noise else 0)
    target = budget + (1 if status == FRESH else 0)
    quiet = engine_noise and not wants
    gflags = 2 if quiet else (1 if engine_noise and status == EXPANDED else 0)
    draw = 1 if engine_noise and not quiet else 0
    return tau, budget, target, gflags, draw, refuse


def _m_line(ply, tau_plies, engine_noise, S, status, sims, noise):
    s, n = sims or [], noise or []
    return "M %d %d %d %d %d %d %s %d %s" % (ply, -1 if tau_plies is None else tau_plies, engine_noise, S, status, len(s),
                                             " ".join(map(str, s)), len(n), " ".join(map(str, n)))


def cadence(turn_every, early, steps):
    out = ""
    while len(out) < steps:
        out += "L" * (turn_every - 1) + ("K" if early else "") + "L" + "T"
    return out[:steps]


# ---- the next move of a game -------------------------------------------------------------------------------------------------------
NEXT_MOVE = {
    # no tables: the engine's S and noise; an inherited, expanded root is re-noised (flag 1) and pays for a draw
    "plain": ((3, 2, 1, 40, EXPANDED, None, None), "M 0 40 40 1 1 0"),
    # tau is 1 while ply < tau_plies
    "tau_last_ply": ((1, 2, 1, 40, EXPANDED, None, None), "M 1 40 40 1 1 0"),
    "tau_always": ((70, None, 1, 40, EXPANDED, None, None), "M 1 40 40 1 1 0"),
    # a fresh root runs its own expansion on top of the budget, and its noise comes at the expansion: no re-noise flag
    "fresh_bonus": ((0, 2, 1, 40, FRESH, [4, 8, 16], None), "M 1 4 5 0 1 0"),
    "known_unexpanded": ((1, 2, 1, 40, KNOWN, [4, 8, 16], None), "M 1 8 8 0 1 0"),
    # a ply beyond the stride reads the last column, of the budgets and of the switches alike
    "beyond_stride": ((9, 2, 1, 40, EXPANDED, [4, 8, 16], [1, 0]), "M 0 16 16 2 0 0"),
    # a quiet game on a noise engine: flag 2, no draw, whatever its root
    "quiet_fresh": ((0, 0, 1, 40, FRESH, None, [0]), "M 0 40 41 2 0 0"),
    "quiet_then_noisy": ((1, 0, 1, 40, EXPANDED, None, [0, 1]), "M 0 40 40 1 1 0"),
    # an engine without noise: no flag, no draw
    "no_noise_engine": ((5, 2, 0, 40, EXPANDED, [7], [0]), "M 0 7 7 0 0 0"),
    # refused: budgets outside 1..S, noise asked of an engine created without it
    "budget_zero": ((0, 2, 1, 40, FRESH, [0], None), "M 1 0 1 0 1 1"),
    "budget_above": ((2, 2, 1, 40, EXPANDED, [4, 8, 41], None), "M 0 41 41 1 1 1"),
    "noise_refused": ((0, 2, 0, 40, FRESH, None, [1]), "M 1 40 41 0 0 2"),
}


@pytest.mark.parametrize("name", sorted(NEXT_MOVE))
def test_next_move_by_hand(program, name):
    args, expect = NEXT_MOVE[name]
    assert "M %d %d %d %d %d %d" % next_move(*args) == expect          # the restatement against the hand-written answer
    assert program([_m_line(*args)])[0] == expect


def test_next_move_random(program):
    rng = np.random.default_rng(31)
    cases = []
    for _ in range(600):
        S = int(rng.integers(1, 401))
        sims = None if rng.random() < 0.3 else [int(x) for x in rng.integers(0, S + 2, size=int(rng.integers(1, 7)))]
        noise = None if rng.random() < 0.3 else [int(x) for x in rng.integers(0, 2, size=int(rng.integers(1, 7)))]
        cases.append((int(rng.integers(0, 12)), None if rng.random() < 0.2 else int(rng.integers(0, 8)), int(rng.integers(0, 2)), S,
                      int(rng.integers(0, 3)), sims, noise))
    got = program([_m_line(*c) for c in cases])
    for c, line in zip(cases, got):
        assert line == "M %d %d %d %d %d %d" % next_move(*c), c


# ---- who turns, drain, when a run returns --------------------------------------------------------------------------------------------
def test_who_turns(program):
    cases = [(i, d, t, l) for i in (0, 1) for d in (0, 3, 4, 5) for t in (0, 4) for l in (0, 1)]
    got = program(["T %d %d %d %d" % c for c in cases])
    for (in_move, done, target, idle), line in zip(cases, got):
        assert line == "T %d" % (1 if in_move and idle and done == target else 0), (in_move, done, target, idle)
    # by hand: finished and idle turns; a leaf under way, a game short of its target or past it, a game outside a move do not
    assert program(["T 1 4 4 1", "T 1 4 4 0", "T 1 3 4 1", "T 1 5 4 1", "T 0 4 4 1", "T 1 0 0 1"]) == ["T 1", "T 0", "T 0", "T 0", "T 0", "T 1"]


def test_drain(program):
    # a turned game begins its next move unless its game is over (win 1, 2, 3) or the roll is draining
    assert program(["B 0 0", "B 0 1", "B 1 0", "B 2 0", "B 3 0", "B 3 1"]) == ["B 1", "B 0", "B 0", "B 0", "B 0", "B 0"]


def test_run_returns(program):
    cases = [(r, m, l, x) for r in (0, 1, 5) for m in (0, 1, 7) for l in (0, 15, 16, 17) for x in (0, 16)]
    got = program(["R %d %d %d %d" % c for c in cases])
    for (records, in_move, launches, bound), line in zip(cases, got):
        assert line == "R %d" % (1 if records > 0 or in_move == 0 or (bound > 0 and launches >= bound) else 0), (records, in_move, launches, bound)
    # by hand: a record; nothing in a move; the bound spent; none of them; no bound however many launches
    assert program(["R 1 7 3 0", "R 0 0 3 0", "R 0 7 16 16", "R 0 7 15 16", "R 0 7 100000 0"]) == ["R 1", "R 1", "R 1", "R 0", "R 0"]


# ---- look / launch / turn ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turn_every", [1, 4, 16])
@pytest.mark.parametrize("early", [0, 1])
def test_cadence(program, turn_every, early):
    steps = 3 * (turn_every + 2) + 1
    line = program(["C %d %d %d" % (turn_every, early, steps)])[0].split()[1]
    assert line == cadence(turn_every, early, steps)
    assert line.count("T") >= 2
    for period in line.split("T")[:-1]:
        assert period.count("L") == turn_every                       # turn_every launches between two turns
        assert period.count("K") == early
        if early:
            assert period.endswith("KL")                             # look, one launch, turn: a settled game idles in no launch


def test_cadence_by_hand(program):
    assert program(["C 1 1 6", "C 1 0 6", "C 4 1 12", "C 4 0 10"]) == ["C KLTKLT", "C LTLTLT", "C LLLKLTLLLKLT", "C LLLLTLLLLT"]
    assert program(["C 16 1 18"])[0] == "C " + "L" * 15 + "KLT"


# ---- the entry points exist ------------------------------------------------------------------------------------------------------------
def test_roll_entry_points():
    from alpha_omok_amd import _lib
    from alpha_omok_amd.engine import Engine
    for name in ("roll_begin", "roll_run", "roll_join", "roll_drain", "roll_end", "roll_stats"):
        assert callable(getattr(Engine, name)), name
        assert "ao_" + name in _lib.SYMBOLS
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    for name in ("ao_roll_begin", "ao_roll_run", "ao_roll_join", "ao_roll_drain", "ao_roll_end", "ao_roll_opts", "ao_roll_records"):
        assert name in hdr
    fields = [f[0] for f in _lib.AoRollOpts._fields_]
    assert fields == ["active", "tau_plies", "sims", "sims_stride", "noise", "noise_stride", "early_stop", "turn_every", "want_visit", "want_policy"]
