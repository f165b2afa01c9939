"""No GPU: the declarations and host-side argument checks of the fp16 forward at every batch size
(AO_NET_PRECISION_FP16_ALL / Net.precision("fp16-all"); the kernels are tested in tests/test_gpu_fp16_all.py), and the batches
those GPU tests draw."""
import os
import re

import numpy as np
import pytest

import fp16_all_batches as fb
import fp16_forward_nets as fn

ROOT = os.path.join(os.path.dirname(__file__), "..")


def test_header_appends_fp16_all_and_keeps_the_signature():
    import ctypes as C
    from alpha_omok_amd import _lib
    src = open(os.path.join(ROOT, "include", "omok_hip.h")).read()
    assert re.search(r"enum\s*\{\s*AO_NET_PRECISION_FP32\s*=\s*0\s*,\s*AO_NET_PRECISION_FP16\s*=\s*1\s*,\s*AO_NET_PRECISION_FP16_ALL\s*=\s*2\s*\}", src)
    m = re.search(r"int\s+ao_net_precision\s*\(([^)]*)\)\s*;", src)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["ao_net *n", "int32_t request", "int32_t *in_force", "int32_t *supported"]
    restype, argtypes = _lib.SYMBOLS["ao_net_precision"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    assert re.search(r"#define\s+AO_ABI_VERSION\s+2\b", src)             # additive: the ABI version stays


def test_net_precisions_has_the_third_string_at_the_enums_index():
    from alpha_omok_amd.engine import Net
    assert Net.PRECISIONS == ("fp32", "fp16", "fp16-all")


def test_configure_accepts_fp16_all_also_with_reproducible(monkeypatch):
    """Argument checks found before any device call: "fp16-all" is one arithmetic for every batch size under mode 6, so it goes
    with reproducible=True; "fp16" still does not. configure() calls train_join() right after its argument checks: it is made to
    raise here, so that reaching it shows the arguments were accepted and nothing of the module's state is touched."""
    import alpha_omok_amd.main as main

    class Accepted(Exception):
        pass

    def stop():
        raise Accepted()

    monkeypatch.setattr(main, "train_join", stop)
    for kw in (dict(), dict(reproducible=True)):
        with pytest.raises(Accepted):
            main.configure(board_size=9, n_mcts=8, n_blocks=2, out_planes=128, forward_precision="fp16-all", **kw)
    with pytest.raises(Accepted):
        main.configure(board_size=9, n_mcts=8, n_blocks=2, out_planes=128, forward_precision="fp16")
    with pytest.raises(ValueError, match="reproducible"):
        main.configure(board_size=9, n_mcts=8, n_blocks=2, out_planes=128, forward_precision="fp16", reproducible=True)
    with pytest.raises(ValueError, match="forward_precision"):
        main.configure(board_size=9, n_mcts=8, n_blocks=2, out_planes=128, forward_precision="bf16")


def test_evaluate_batched_accepts_fp16_all_alone_and_in_a_pair():
    from alpha_omok_amd import evaluate
    assert evaluate.check_forward_precision("fp16-all") == ("fp16-all", "fp16-all")
    assert evaluate.check_forward_precision(("fp16-all", "fp32")) == ("fp16-all", "fp32")
    assert evaluate.check_forward_precision(None) == (None, None)
    for bad in ("bf16", ("fp16-all",), ("fp16-all", "fp8")):
        with pytest.raises(ValueError, match="forward_precision"):
            evaluate.check_forward_precision(bad)
    with pytest.raises(ValueError, match="forward_precision"):           # evaluate_batched itself: the check comes before any device call
        evaluate.evaluate_batched(None, None, 9, 8, forward_precision="bf16")


@pytest.mark.parametrize("module,flag", [("alpha_omok_amd/main.py", "'--fp16-forward-all'"), ("tools/train_omok.py", '"--fp16-forward-all"')])
def test_cli_flag_is_declared_mutually_exclusive_with_fp16_forward(module, flag):
    src = open(os.path.join(ROOT, module)).read()
    g = re.search(r"(\w+) = ap\.add_mutually_exclusive_group\(\)", src)
    assert g, module
    assert re.search(r"%s\.add_argument\(%s" % (g.group(1), re.escape(flag)), src)
    assert re.search(r"%s\.add_argument\(%s" % (g.group(1), re.escape(flag.replace("-all", ""))), src)


def test_batches_of_the_new_shapes_hold_distinct_binary_boards():
    for nb, B, batch in fb.SHAPES:
        idx = fb.batch_of(B, batch)
        x = fn.binary_pool(B)
        assert idx.shape == (batch,) and idx.min() >= 0 and idx.max() < len(x)
        assert len(np.unique(idx)) >= min(16, len(x) // 2), (B, batch, len(np.unique(idx)))
        assert np.array_equal(idx[:5], fn.batch_of(B, batch)[:5])        # the structured boards stay at the head of the batch
