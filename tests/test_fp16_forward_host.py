"""No GPU: the conditions of the fp16-forward test networks from the float64 reference alone, the host-side argument checks of
main.configure(forward_precision=) and the ctypes declaration of ao_net_precision.

The GPU tests (tests/test_gpu_fp16_forward.py) assert BIT equalities between the one-product kernels and the default forward.
Those equalities are properties of the networks of tests/fp16_forward_nets.py; they are established here, on the CPU, in float64:
  * the library's BatchNorm fold returns the weights themselves (so the device and the reference multiply by the same numbers);
  * every activation the reference stores on the exact network is an fp16 number (rounding to fp16 is then the identity);
  * on the perturbed twin, rounding every stored activation to fp16 (to nearest) gives the unperturbed network's result exactly,
    and not rounding gives something else.
"""
import os
import re

import numpy as np
import pytest

import fp16_forward_nets as fn
import net_reference as nr

SHAPES = [(2, 3), (1, 3), (2, 4), (1, 7), (2, 9), (2, 10), (1, 12), (2, 15)]       # (blocks, board): the recipe's shapes and every shape of the GPU tests


@pytest.mark.parametrize("nb,B", SHAPES)
def test_exact_network_stores_fp16_numbers_only(nb, B):
    import torch
    sd = fn.exact_network(nb, B)
    assert fn.fold_is_exact(sd)
    x = fn.binary_pool(B)
    assert len(x) >= 32 and set(np.unique(x)) <= {0.0, 1.0}
    o, acts = fn.spy_forward(sd, x)
    assert len(acts) == 1 + 2 * nb
    for a in acts:
        assert bool((a.to(torch.float16).double() == a).all())
        assert float(a.max()) <= 2048.0                       # far inside the fp16 range: no clamp, no range event
        assert 0.2 <= float((a > 0).double().mean()) <= 0.8   # live: a defect is not hidden behind dead ReLUs
    # ... so the "fp16 forward" of the definition is the plain forward on this network
    o16 = nr.forward(fn.as_folded(sd), x, act_round=fn.r16)
    assert torch.equal(o16["logits"], o["logits"]) and torch.equal(o16["z"], o["z"])
    # usable priors for a search: no vanishing move, no saturated value
    p = torch.softmax(o["logits"], dim=1)
    assert p.min().item() >= 1e-7 and o["z"].abs().max().item() <= 1.5
    # the conv weights are fp16 numbers: the default forward of this network is the two-product form
    assert all(np.array_equal(v, v.astype(np.float16).astype(np.float32)) for v in sd.values() if v.ndim == 4 and v.shape[2] == 3)


@pytest.mark.parametrize("nb,B", [(2, 9), (1, 7), (2, 15), (2, 10)])
def test_perturbed_twin_is_restored_by_rounding_to_nearest_and_by_nothing_else(nb, B):
    import torch
    twin, pert = fn.perturbed_pair(nb, B)
    assert fn.fold_is_exact(twin) and fn.fold_is_exact(pert)
    x = fn.binary_pool(B)
    o_twin = nr.forward(fn.as_folded(twin), x)
    o_twin16 = nr.forward(fn.as_folded(twin), x, act_round=fn.r16)
    assert torch.equal(o_twin["trunk"], o_twin16["trunk"])                        # the twin is still exact
    fast = nr.forward(fn.as_folded(pert), x, act_round=fn.r16)
    assert torch.equal(fast["trunk"], o_twin["trunk"]) and torch.equal(fast["logits"], o_twin["logits"]) and torch.equal(fast["z"], o_twin["z"])
    full = nr.forward(fn.as_folded(pert), x)
    dl, dz = nr.distances(full, o_twin)
    assert 5e-4 <= dl <= 1e-1, (dl, dz)                                           # measured: 2e-3 .. 3e-2 in a logit
    # truncation instead of rounding to nearest does NOT restore the twin

    def trunc16(t):
        h = t.to(torch.float16)
        h = torch.where(h.to(t.dtype) > t, torch.nextafter(h, torch.zeros_like(h)), h)
        return h.to(t.dtype)

    tr = nr.forward(fn.as_folded(pert), x, act_round=trunc16)
    assert not torch.equal(tr["trunk"], o_twin["trunk"])


def test_batches_are_drawn_from_the_binary_boards():
    for B, batch in [(9, 3073), (7, 3104), (4, 3073), (3, 3072), (15, 65), (10, 64), (12, 65)]:
        idx = fn.batch_of(B, batch)
        x = fn.binary_pool(B)
        assert idx.shape == (batch,) and idx.min() >= 0 and idx.max() < len(x)
        assert len(np.unique(idx)) >= min(16, len(x) // 2)


def test_configure_checks_forward_precision_on_the_host():
    """Both are argument errors found before any device call: this test runs without a GPU."""
    import alpha_omok_amd.main as main
    with pytest.raises(ValueError, match="forward_precision"):
        main.configure(board_size=9, n_mcts=8, n_blocks=2, out_planes=128, forward_precision="bf16")
    with pytest.raises(ValueError, match="reproducible"):
        main.configure(board_size=9, n_mcts=8, n_blocks=2, out_planes=128, forward_precision="fp16", reproducible=True)


def test_lib_declares_ao_net_precision_with_the_headers_signature():
    import ctypes as C
    from alpha_omok_amd import _lib
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "omok_hip.h")).read()
    m = re.search(r"int\s+ao_net_precision\s*\(([^)]*)\)\s*;", src)
    assert m, "ao_net_precision is not declared in include/omok_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["ao_net *n", "int32_t request", "int32_t *in_force", "int32_t *supported"]
    restype, argtypes = _lib.SYMBOLS["ao_net_precision"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    assert re.search(r"AO_NET_PRECISION_FP32\s*=\s*0\s*,\s*AO_NET_PRECISION_FP16\s*=\s*1", src)
    assert re.search(r"ao_abi_version", src)
