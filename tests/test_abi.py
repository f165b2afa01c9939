"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol the header declares."""
import ctypes
import os
import re

from conftest import REPO


def test_library_exports_every_declared_symbol():
    from alpha_omok_amd import _lib, build
    path = build.build()
    assert os.path.exists(path)
    lib = _lib.load(build_if_missing=False)
    hdr = open(os.path.join(REPO, "include", "omok_hip.h")).read()
    declared = set(re.findall(r"\b(ao_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"ao_engine", "ao_net", "ao_config"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), "libomok_hip.so does not export %s" % name
    assert set(_lib.SYMBOLS) == declared
    assert lib.ao_abi_version() == 2
    assert b"gfx950" in lib.ao_version()


def test_create_fails_loudly_without_gpu():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from alpha_omok_amd.engine import Engine, EngineError
    with pytest.raises(EngineError):
        Engine(9, 10, 5, games=1)


_CREATES_WITH_DEVICE_9999 = r"""
import ctypes, json
from alpha_omok_amd import _lib
lib = _lib.load(build_if_missing=False)
DEV = 9999
cfg = _lib.AoConfig(board=9, win_mark=5, sims=8, inplanes=5, games=2, noise=1, node_cap=0, device=DEV, c_puct=0.0, alpha=0.0,
                    arena_fraction=0.0)
rcfg = _lib.AoRolloutConfig(board=9, win_mark=5, sims=8, games=2, mode=0, device=DEV, c_puct=0.0)
tcfg = _lib.AoTttConfig(board=3, win_mark=3, sims=8, games=2, device=DEV)
creates = [
    ("ao_create", lambda h: lib.ao_create(ctypes.byref(cfg), h), lib.ao_last_error),
    ("ao_net_create", lambda h: lib.ao_net_create(1, 5, 32, 9, DEV, h), lib.ao_net_last_error),
    ("ao_replay_create", lambda h: lib.ao_replay_create(9, 5, 64, DEV, h), lib.ao_replay_last_error),
    ("ao_rollout_create", lambda h: lib.ao_rollout_create(ctypes.byref(rcfg), h), lib.ao_rollout_last_error),
    ("ao_ttt_create", lambda h: lib.ao_ttt_create(ctypes.byref(tcfg), h), lib.ao_ttt_last_error),
    ("ao_positions_create", lambda h: lib.ao_positions_create(9, 5, 5, 16, DEV, h), lib.ao_positions_last_error),
]
res = {}
for name, create, last_error in creates:
    out = ctypes.c_void_p(1)   # (not NULL: the call itself must clear it)
    rc = create(ctypes.byref(out))
    res[name] = [rc, out.value, last_error(None).decode()]
print(json.dumps(res))
"""


def test_every_create_turns_an_invalid_device_away():
    """Every ao_*_create with otherwise valid arguments and device ordinal 9999: non-zero, *out NULL, a message behind
    *_last_error(NULL) -- with the entry point's name in front where the Python wrapper does not add it. The ordinal is refused
    before any device is touched, so this runs with and without a GPU; the rest of the text is the HIP runtime's. In a process
    of its own: a refused hipSetDevice stays behind as the thread's last HIP error, which torch would report at its next launch."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _CREATES_WITH_DEVICE_9999], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    prefixes = {"ao_create": "", "ao_net_create": "", "ao_replay_create": "ao_replay_create: ", "ao_rollout_create": "ao_rollout_create: ",
                "ao_ttt_create": "ao_ttt_create: ", "ao_positions_create": "ao_positions_create: "}
    assert sorted(res) == sorted(prefixes)
    for name, (rc, out, msg) in res.items():
        print("%s: %r" % (name, msg))
        assert rc != 0, name
        assert out is None, name
        assert msg.startswith(prefixes[name]) and len(msg) > len(prefixes[name]), (name, msg)


def test_host_thread_budget_follows_local_world_size():
    """ao_host_threads: the per-process pool for the per-move Dirichlet replay is hardware threads / LOCAL_WORLD_SIZE
    (torchrun's variable: the ranks of a node share the host), at most 32, at least 1; AO_HOST_THREADS overrides."""
    import subprocess
    import sys
    hw = os.cpu_count() or 1
    code = "from alpha_omok_amd import _lib; print(_lib.load(build_if_missing=False).ao_host_threads())"

    def ask(**env):
        e = {k: v for k, v in os.environ.items() if k not in ("LOCAL_WORLD_SIZE", "AO_HOST_THREADS")}
        e.update(env)
        return int(subprocess.run([sys.executable, "-c", code], env=e, cwd=REPO, capture_output=True, text=True,
                                  check=True).stdout.strip().splitlines()[-1])

    assert ask() == max(1, min(32, hw))
    assert ask(LOCAL_WORLD_SIZE="8") == max(1, min(32, hw // 8))
    assert ask(LOCAL_WORLD_SIZE="8", AO_HOST_THREADS="3") == 3
