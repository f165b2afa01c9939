"""Networks that leave the fp16 range WITHOUT saturating, and the boards that do and do not take them there: what
tests/test_fp16_range_host.py (CPU), tests/test_gpu_fp16_range.py and tests/test_gpu_fp16_range_search.py (GPU) share.

The split-fp16 kernels store every trunk activation as fp16 halves: a value above 65504 is clamped and the network's status
word gets AO_NET_FP16_RANGE. A test of that report needs a network whose activations leave the range while its OUTPUTS stay
ordinary (bn1.weight * 3e5, the one earlier construction, saturates the policy a ply later). The constructions here are built
on net_reference.case_network(...) and scale ONE channel whose readers have zero weights:

  * dead channel, inner: layers.k.bn1 weight and bias of channel c times 2^20, layers.k.conv2.weight[:, c] = 0. The inner
    activation of block k overflows on channel c; nothing reads it.
  * dead channel, last:  the same on bn2 of the last block; input channel c of both head 1x1 convs zeroed.
  * dead channel, stem:  the same on bn1; [:, c] of every block's conv1 and of both head convs zeroed. The skip connection
    carries the overflow through every residual store, so every layer of the trunk writes it.
  * stem detector:       conv1.weight[c] is the centre tap of input plane 0 alone (1.0), bn1 folds to scale k and shift 0 on
    channel c, which is dead downstream as in "stem". A value of 1.0 at one (board, cell) of plane 0 gives ONE activation of
    exactly k at that board, cell and channel (and k + O(1) in every residual store of that channel after it); a board whose
    plane 0 is empty gives 0 there.

`scale=1` of a dead-channel construction is the DEAD network: the channel cut off, nothing scaled. Big and dead networks are the
same function (a clamped or unclamped activation times a zero weight is 0.0), so the float64 evaluation of the dead network is
also the reference of a clamping kernel. Every construction only zeroes conv weights or writes 1.0: weights on the fp16 grid
stay there.

A board is OVER when some stored activation (net_reference.forward's act_round hook sees exactly the stored ones) is above
2 x 65504 and UNDER when every one is below 65504 / 2; nothing in the tests depends on a value in between, except the two
detector values 70000 (must be reported) and 60000 (must not)."""
import functools

import numpy as np

import net_reference as R

LIMIT = 65504.0
K_DEAD = float(2 ** 20)
CH = 77
KINDS = ("inner", "last", "stem")
DETECT_OVER, DETECT_IN = 70000.0, 60000.0
HEADS = ("policy_head.policy_head.weight", "value_head.value_head.weight")


def _zero_inputs(sd, key, c):
    w = np.array(sd[key], copy=True)
    w[:, c] = 0
    sd[key] = w


def dead_channel(sd, kind, c=CH, block=0, scale=K_DEAD):
    """`sd` with channel c of one BatchNorm scaled by `scale` and cut off from everything that reads it (this module's docstring).
    kind: "inner" (bn1 of block `block`), "last" (bn2 of the last block) or "stem" (bn1). scale=1: the dead network."""
    sd = dict(sd)
    nb = R.n_blocks(sd)
    assert nb >= 1 and kind in KINDS
    if kind == "inner":
        bn = "layers.%d.bn1" % block
        _zero_inputs(sd, "layers.%d.conv2.weight" % block, c)
    elif kind == "last":
        bn = "layers.%d.bn2" % (nb - 1)
    else:
        bn = "bn1"
        for i in range(nb):
            _zero_inputs(sd, "layers.%d.conv1.weight" % i, c)
    if kind != "inner":
        for k in HEADS:
            _zero_inputs(sd, k, c)
    for p in (".weight", ".bias"):
        v = np.array(sd[bn + p], copy=True)
        v[c] = v[c] * np.float32(scale)
        sd[bn + p] = v
    return sd


def stem_detector(sd, c, k):
    """The stem detector on channel c with folded scale k (this module's docstring). running_var is the float32 nearest to
    1 - 1e-5, so that the library's fold k / sqrt(var + 1e-5), computed in double and cast to float, is k itself."""
    sd = dead_channel(sd, "stem", c, scale=1.0)
    w = np.array(sd["conv1.weight"], copy=True)
    w[c] = 0
    w[c, 0, 1, 1] = 1.0
    sd["conv1.weight"] = w
    for p, val in ((".weight", k), (".bias", 0.0), (".running_mean", 0.0), (".running_var", 1.0 - 1e-5)):
        v = np.array(sd["bn1" + p], copy=True)
        v[c] = np.float32(val)
        sd["bn1" + p] = v
    assert np.float32(float(k) / np.sqrt(np.float64(sd["bn1.running_var"][c]) + 1e-5)) == np.float32(k)
    return sd


def stored_peaks(sd, x):
    """[boards]: the largest activation the trunk stores for each board of x (float64 reference, nothing clamped)."""
    import torch
    peaks = []

    def spy(t):
        peaks.append(t.flatten(1).max(dim=1).values)
        return t

    R.forward(sd, x, act_round=spy)
    assert len(peaks) == 1 + 2 * R.n_blocks(sd)
    return torch.stack(peaks).max(dim=0).values.numpy()


def clamp(t):
    import torch
    return torch.clamp(t, max=LIMIT)


@functools.lru_cache(maxsize=None)
def big_network(nb, B, kind, grid=False, c=CH):
    return dead_channel(R.case_network(nb, B, 128, grid), kind, c)


@functools.lru_cache(maxsize=None)
def dead_network(nb, B, kind, grid=False, c=CH):
    return dead_channel(R.case_network(nb, B, 128, grid), kind, c, scale=1.0)


@functools.lru_cache(maxsize=None)
def kinds_of_pool(nb, B, kind, grid=False):
    """(over, under): boolean masks over net_reference.pool(B) under big_network(nb, B, kind, grid). Read-only."""
    pk = stored_peaks(big_network(nb, B, kind, grid), R.pool(B))
    over, under = pk > 2 * LIMIT, pk < LIMIT / 2
    over.setflags(write=False)
    under.setflags(write=False)
    return over, under


def r16(t):
    """the stored activation of the one-product kernels: clamped, rounded once to fp16 (fp16_forward_nets.r16)"""
    import torch
    return torch.clamp(t, max=LIMIT).to(torch.float16).to(t.dtype)


def reference(sd, x, f16=False):
    """The float64 evaluation of `sd` on planes x as float64 numpy arrays `logits` (centred) and `z`, and per board the distance
    `ul` / `uz` of the evaluation the bound's unit is measured with: the same plain evaluation in float32 (E32, as
    net_reference.units), or -- f16 -- the host emulation of the one-product forward (fp16 conv weights, every stored
    activation rounded once: E_fast of tests/test_gpu_fp16_forward.py)."""
    import torch
    exact = R.forward(sd, x)
    other = R.forward(R.project_to_fp16_grid(sd), x, act_round=r16) if f16 else R.forward(sd, x, torch.float32)
    le, lo = R.centred(exact["logits"].double()), R.centred(other["logits"].double())
    return dict(logits=le.numpy(), z=exact["z"].double().numpy(), ul=(lo - le).abs().max(dim=1).values.numpy(),
                uz=(other["z"].double() - exact["z"].double()).abs().numpy())


def fp16_planes(x):
    return np.all(x.astype(np.float16).astype(np.float32) == x, axis=(1, 2, 3))


@functools.lru_cache(maxsize=None)
def dead_reference(nb, B, kind, grid=False, f16=False):
    """reference(...) of dead_network(nb, B, kind, grid) on net_reference.pool(B)"""
    return reference(dead_network(nb, B, kind, grid), R.pool(B), f16)


@functools.lru_cache(maxsize=None)
def detector_reference(nb, B, grid, c, f16=False):
    """reference(...) of the in-range stem detector on channel c on quiet_pool(B)"""
    return reference(stem_detector(R.case_network(nb, B, 128, grid), c, DETECT_IN), quiet_pool(B), f16)


@functools.lru_cache(maxsize=None)
def detector_board_reference(nb, B, grid, c, cell, f16=False):
    return reference(stem_detector(R.case_network(nb, B, 128, grid), c, DETECT_IN), detector_board(B, cell)[None], f16)


def unit(ref, boards, f16=False):
    """(unit of the centred logits, unit of z) over the pool boards `boards`: the largest per-board distance, with
    net_reference's floor where the unit is E32"""
    u = np.unique(boards)
    floor = 0.0 if f16 else R.E32_FLOOR
    return max(float(ref["ul"][u].max()), floor), max(float(ref["uz"][u].max()), floor)


def batch(fam):
    """Pool indices of a family's batch: net_reference.batch_indices' draw (over boards on every shape and kind, asserted by
    tests/test_fp16_range_host.py); for the one-product forms the boards whose planes are no fp16 numbers replaced by random
    boards that are, as tests/test_gpu_fp16_forward.py does."""
    m = R.batch_indices(fam.batch, fam.B)
    if fam.precision != "fp32":
        ok = fp16_planes(R.pool(fam.B))
        repl = np.random.RandomState(fam.batch).choice(np.nonzero(ok)[0], size=fam.batch)
        m = np.where(ok[m], m, repl)
    return m


def under_batch(fam, kind):
    """Pool indices of a batch of the family's size made of UNDER boards alone, every under board of the pool in it."""
    under = np.nonzero(kinds_of_pool(fam.nb, fam.B, kind, fam.grid)[1])[0]
    assert len(under) > 0
    return under[np.arange(fam.batch) % len(under)]


def has_under(B, kind):
    """whether net_reference.pool(B) holds under boards of big_network(2, B, kind): 4x4 for every kind, 10x10 but for "last" """
    return B == 4 or (B == 10 and kind != "last")


# --------------------------------------------------------------------------------------------------------------------------
# the kernel families of the flag: (id, kernel name, blocks, board, batch, trunk mode, environment of Net(), grid, precision)
# --------------------------------------------------------------------------------------------------------------------------
class Family:
    def __init__(self, family, kernel, B, batch, mode=0, env=None, grid=False, precision="fp32", nb=2):
        self.family, self.kernel, self.nb, self.B, self.batch, self.mode = family, kernel, nb, B, batch, mode
        self.env, self.grid, self.precision = dict(env or {}), grid, precision
        self.products = {"fp32": 2 if grid else 3}.get(precision, 1)
        self.id = "%s-B%d-%d" % (kernel.split("<")[0][2:], B, batch) + "".join("-fmt" + v for k, v in self.env.items())
        self.f16 = precision != "fp32"
        # the bound on the outputs: 16 x E32 for the split-fp16 families (net_reference.Case.mult), 3 x E_fast for the one-product
        # forms (tests/test_gpu_fp16_forward.py)
        self.mult = 3 if self.f16 else 16


def _families():
    out = []

    def both(family, kernel, B, batch, mode=0, env=None, w16=True):
        out.append(Family(family, kernel, B, batch, mode, env))
        if w16:
            head, _, tail = kernel.partition("<")
            out.append(Family(family, head + "_w16<" + tail, B, batch, mode, env, grid=True))

    both("conv_cells_h", "k_conv_cells_h<9, 8>", 9, 5)
    both("row16hk", "k_row16hk<9>", 9, 33)
    both("layer16hk4", "k_layer16hk<9, 4>", 9, 760)
    both("layer16h", "k_layer16h<9>", 9, 70, mode=6)
    both("trunk16h_fmt0", "k_trunk16h<9, 4, 0>", 9, 3073, env={"AO_TRUNK_FMT": "0"})
    both("trunk16h_fmt1", "k_trunk16h<9, 4, 1>", 9, 3073, env={"AO_TRUNK_FMT": "1"}, w16=False)
    both("boardh", "k_boardh<10, 1>", 10, 65)
    both("layer16h_wide", "k_layer16h<10>", 10, 63)
    # one even and one odd narrow width besides 9, at the resident trunk and the per-layer kernel (4x4 also holds under boards,
    # so the narrow-board kernels get their "under boards only" batch here: the other 4x4 rungs of net_reference's ladder too)
    both("conv_cells_h", "k_conv_cells_h<4, 8>", 4, 5)
    both("row16hk", "k_row16hk<4>", 4, 300)
    both("layer16hk4", "k_layer16hk<4, 4>", 4, 1000)
    both("layer16h", "k_layer16h<4>", 4, 2000)
    both("trunk16h_fmt0", "k_trunk16h<4, 4, 0>", 4, 3073, env={"AO_TRUNK_FMT": "0"})
    both("layer16h", "k_layer16h<7>", 7, 70, mode=6)
    both("trunk16h_fmt0", "k_trunk16h<7, 4, 0>", 7, 3073, env={"AO_TRUNK_FMT": "0"})
    # the one-product forms of the opt-in fp16 forward
    out.append(Family("trunk16h_f16", "k_trunk16h_f16<9, 4, 0>", 9, 3073, grid=True, precision="fp16"))
    out.append(Family("trunk16h_f16", "k_trunk16h_f16<4, 4, 0>", 4, 3073, grid=True, precision="fp16"))
    out.append(Family("boardh_f16", "k_boardh_f16<10, 1>", 10, 65, grid=True, precision="fp16"))
    out.append(Family("layer16h_f16", "k_layer16h_f16<9>", 9, 70, mode=6, grid=True, precision="fp16-all"))
    out.append(Family("layer16h_f16", "k_layer16h_f16<10>", 10, 63, grid=True, precision="fp16-all"))
    return out


FAMILIES = _families()

# what part A of the issue names: every family, its _w16 form where one exists and the three _f16 forms
NAMED = ["k_conv_cells_h<9, 8>", "k_row16hk<9>", "k_layer16hk<9, 4>", "k_layer16h<9>", "k_trunk16h<9, 4, 0>", "k_trunk16h<9, 4, 1>",
         "k_boardh<10, 1>", "k_layer16h<10>", "k_conv_cells_h_w16<9, 8>", "k_row16hk_w16<9>", "k_layer16hk_w16<9, 4>", "k_layer16h_w16<9>",
         "k_trunk16h_w16<9, 4, 0>", "k_boardh_w16<10, 1>", "k_layer16h_w16<10>", "k_trunk16h_f16<9, 4, 0>", "k_boardh_f16<10, 1>",
         "k_layer16h_f16<9>", "k_trunk16h<4, 4, 0>", "k_trunk16h<7, 4, 0>", "k_layer16h<4>", "k_layer16h<7>"]
# the families that read bit planes have no forward entry point: a search reaches them (board, games, simulations, kernel)
SEARCH_FAMILIES = [(9, 3072, 12, "k_trunk16hb<9, 4, 0>"), (10, 64, 8, "k_boardh<10, 2>"), (9, 5, 16, "k_conv_cells_h<9, 8>")]


# --------------------------------------------------------------------------------------------------------------------------
# the pinpoint sweep of the stem detector
# --------------------------------------------------------------------------------------------------------------------------
CHANNELS = (0, 15, 16, 77, 127)


def sweep_boards(batch):
    """rows {0, 15, 16, the last live row of the ragged group} of a batch (those that exist, once each)"""
    return sorted({r for r in (0, 15, 16, batch - 1) if 0 <= r < batch})


def sweep_cells(B):
    """cells {0, B-1, A-B, A-1, centre}: the four corners and the centre"""
    A = B * B
    return sorted({0, B - 1, A - B, A - 1, (B // 2) * B + B // 2})


def sweep_points(B, batch, limit=40):
    """[(row, cell, channel)] of the detector sweep. The full product of sweep_boards x sweep_cells x CHANNELS (up to 100 points,
    one forward each and two values per point) where the batch is small; at 3073 boards a Latin-square-style subset: point
    (i, j) of boards x cells takes channel (i + 2 j) mod 5 -- 20 points in which every row, every cell and every channel
    appears (each row and each cell with 4 .. 5 channels, each channel 4 times) -- so that with the two values it stays at
    `limit` = 40 forwards."""
    rows, cells = sweep_boards(batch), sweep_cells(B)
    if 2 * len(rows) * len(cells) * len(CHANNELS) <= limit or batch < 3073:
        return [(r, q, c) for r in rows for q in cells for c in CHANNELS]
    pts = [(r, q, CHANNELS[(i + 2 * j) % len(CHANNELS)]) for i, r in enumerate(rows) for j, q in enumerate(cells)]
    assert 2 * len(pts) <= limit
    assert {p[0] for p in pts} == set(rows) and {p[1] for p in pts} == set(cells) and {p[2] for p in pts} == set(CHANNELS)
    return pts


@functools.lru_cache(maxsize=None)
def quiet_pool(B):
    """net_reference.pool(B) with plane 0 emptied: boards on which the detector channel stores 0. Read-only."""
    x = np.array(R.pool(B), copy=True)
    x[:, 0] = 0
    x.setflags(write=False)
    return x


def detector_board(B, cell, base=5):
    """quiet_pool(B)[base] with the one stone of plane 0 at `cell`."""
    b = np.array(quiet_pool(B)[base], copy=True)
    b[0, cell // B, cell % B] = 1.0
    return b
