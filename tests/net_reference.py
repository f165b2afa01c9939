"""A plain float64 evaluation of PVNet from a state_dict, conditioned test networks, and inputs that reach the edges:
what tests/test_net_reference.py (CPU) and tests/test_gpu_net_precision.py (GPU) share.

Why a second weight generator exists. `pvnet_weights.make_state_dict` (kept as it is: tools/gen_golden.py and the committed
fixtures depend on it) draws He-initialised convs and BatchNorms that do not normalise, so a residual tower doubles its
activation variance per block. Evaluated in float64 on the batches of test_gpu_net.test_forward_vs_torch_fp32 this gives
(`saturation_table()` below regenerates the rows; profiles/r7a_forward_precision_by_family.txt keeps a copy):

    (nb, B, planes, batch)   distinct v    1 - |v|                        share of p < 1e-6   median max p
    (4, 9, 128, 70)          1 of 70       0.83 for every board           0.50                0.73
    (10, 9, 128, 33)         1 of 33       <= 1.9e-8 (tanh saturated)     0.75                0.85
    (1, 3, 128, 3)           2 of 3        --                             0                   0.69
    (3, 9, 64, 32)           32 of 32      down to 1.1e-3                 0.18                0.96
    the other four           all distinct  healthy                        0                   0.07 .. 0.14

On the two 9x9 / 128-plane rows the value head's ReLU is dead on every cell of every board: v is a constant, and the value
1x1 conv, value_fc1 and all of the trunk that feeds them could return anything without moving it. The policy is close to
one-hot, so an absolute 1e-4 on p sees two or three logits of a board. `conditioned_state_dict` returns networks on which the
heads are live and the tower stays O(1), and the comparison moves to logit space (centred log p, atanh v), where its unit is
the float32-vs-float64 distance of this same plain evaluation.
"""
import functools

import numpy as np

import pvnet_weights

EPS = 1e-5          # torch.nn.BatchNorm2d's default eps (model.py builds its BatchNorms with the default)
POOL = 96           # boards of a pool (9x9 and smaller); WIDE_POOL for boards wider than 9
WIDE_POOL = 48


# ------------------------------------------------------------------------------------------------------------------
# 1. the plain reference
# ------------------------------------------------------------------------------------------------------------------
def n_blocks(sd):
    nb = 0
    while "layers.%d.conv1.weight" % nb in sd:
        nb += 1
    return nb


def forward(sd, x, dtype=None, act_round=None, resume=None, trunk=None):
    """PVNet in eval() mode from `sd` (name -> numpy array, the reference's key names), evaluated in `dtype` (float64 unless
    told otherwise) with nothing but conv2d, the affine form of BatchNorm on its running statistics, ReLU and matmul.
    Returns a dict of torch tensors: `logits` [batch, A] (before the softmax), `z` [batch] (before the tanh), `trunk` (the
    tower's output), `hp` / `hv` (the two head activations after their ReLU, flattened NCHW), `h1` (value_fc1 after its ReLU)
    and `last_in` (the input of the last ResBlock, or of the heads when there is no block).
    act_round: a function applied to every activation the trunk stores between layers (the defect catalogue's "one fp16").
    resume: a `last_in` tensor of an earlier call with the same trunk below the last block: only the last block and the heads
    are evaluated. trunk: a `trunk` tensor of an earlier call with the same trunk weights: only the heads are evaluated."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    if trunk is not None:
        resume = trunk

    def g(k):
        return torch.from_numpy(np.asarray(sd[k])).to(dtype)

    def bn(y, p):
        sc = g(p + ".weight") / torch.sqrt(g(p + ".running_var") + EPS)
        sh = g(p + ".bias") - g(p + ".running_mean") * sc
        return y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)

    r = act_round or (lambda t: t)
    nb = n_blocks(sd)

    def block(i, t):
        y = r(F.relu(bn(F.conv2d(t, g("layers.%d.conv1.weight" % i), padding=1), "layers.%d.bn1" % i)))
        return r(F.relu(bn(F.conv2d(y, g("layers.%d.conv2.weight" % i), padding=1), "layers.%d.bn2" % i) + t))

    with torch.no_grad():
        if resume is None:
            t = r(F.relu(bn(F.conv2d(torch.from_numpy(np.array(x, np.float32)).to(dtype), g("conv1.weight"), padding=1), "bn1")))
            for i in range(nb - 1):
                t = block(i, t)
        else:
            t = resume.to(dtype)
        last_in = t
        if nb and trunk is None:
            t = block(nb - 1, t)
        elif trunk is not None:
            t = trunk.to(dtype)
        hp = F.relu(bn(F.conv2d(t, g("policy_head.policy_head.weight")), "policy_head.policy_bn")).flatten(1)
        logits = hp @ g("policy_head.policy_fc.weight").T + g("policy_head.policy_fc.bias")
        hv = F.relu(bn(F.conv2d(t, g("value_head.value_head.weight")), "value_head.value_bn")).flatten(1)
        h1 = F.relu(hv @ g("value_head.value_fc1.weight").T + g("value_head.value_fc1.bias"))
        z = (h1 @ g("value_head.value_fc2.weight").T + g("value_head.value_fc2.bias")).squeeze(-1)
    return dict(logits=logits, z=z, trunk=t, hp=hp, hv=hv, h1=h1, last_in=last_in)


def centred(l):
    """logits (or log p) minus their mean over a board's moves: what a softmax leaves of them."""
    return l - l.mean(dim=1, keepdim=True)


def distances(a, b):
    """(max |centred logits of a - of b|, max |z of a - of b|) in float64, over the batch."""
    import torch
    dl = (centred(a["logits"].to(torch.float64)) - centred(b["logits"].to(torch.float64))).abs().max().item()
    dz = (a["z"].to(torch.float64) - b["z"].to(torch.float64)).abs().max().item()
    return dl, dz


# ------------------------------------------------------------------------------------------------------------------
# 3. inputs that reach the edges
# ------------------------------------------------------------------------------------------------------------------
def structured_boards(B, C=5):
    """Boards a kernel's halo, padding and group handling can get wrong, as [n, C, B, B] float32, and their names. Planes
    0 .. C-2 are stones (of the player to move and of the opponent, present and past), plane C-1 the colour to move.
    C = 1 (ao_net_create takes it; no history depth gives it) has no room for both: there the one plane carries the stones
    and the sparse float values, and is constant only on the two "empty" boards (on constant planes alone a network of one
    input plane has five distinct results over the whole pool, and conv1 could permute its taps unseen)."""
    m = B // 2
    out, names = [], []

    def add(name, b):
        out.append(b)
        names.append(name)

    add("empty, colour 0", np.zeros((C, B, B), np.float32))
    b = np.zeros((C, B, B), np.float32); b[C - 1] = 1
    add("empty, colour 1", b)
    b = np.zeros((C, B, B), np.float32); b[:C - 1] = 1
    add("full", b)
    for name, (y, x) in (("corner 0,0", (0, 0)), ("corner 0,N", (0, B - 1)), ("corner N,0", (B - 1, 0)), ("corner N,N", (B - 1, B - 1)),
                         ("mid-edge top", (0, m)), ("mid-edge left", (m, 0)), ("mid-edge right", (m, B - 1)), ("mid-edge bottom", (B - 1, m))):
        b = np.zeros((C, B, B), np.float32)
        if C > 1:
            b[C - 1] = len(out) % 2
        b[(len(out) % (C - 1)) if C > 1 else 0, y, x] = 1        # the stone's plane changes from board to board
        add("one stone, " + name, b)
    rs = np.random.RandomState(7000 + B)
    for k in range(3):
        # values that are not 0/1 and not fp16 numbers (ao_net_forward takes any float32 planes: conv1 of the split-fp16
        # kernels must split them in two halves like every other layer's input): N(0, 3^2) as
        # test_split_fp16_forward_takes_arbitrary_float_planes draws them, on 3 .. 8 % of the cells,
        # so the board stays inside what the conditioned networks are conditioned for
        b = (rs.standard_normal((C, B, B)) * 3.0).astype(np.float32)
        b *= (rs.rand(C, B, B) < (0.03, 0.05, 0.08)[k])
        if C > 1:
            b[C - 1] = np.float32(0.37 + 0.21 * k)
        add("float planes %d" % k, b)
    return np.stack(out), names


@functools.lru_cache(maxsize=None)
def pool(B, C=5, n=None, seed=0):
    """The boards every batch of the precision tests is drawn from: the structured boards first, then random 0/1 planes
    (30 % stones per plane, one colour per board) as the existing forward tests draw them. Read-only."""
    n = n or (POOL if B <= 9 else WIDE_POOL)
    s, _ = structured_boards(B, C)
    rs = np.random.RandomState(1000 * B + C + 7919 * seed)
    x = (rs.rand(n, C, B, B) < 0.3).astype(np.float32)
    colour = (rs.rand(n, 1, 1) < 0.5).astype(np.float32)
    if C > 1:
        x[:, C - 1] = colour
    k = min(len(s), n)
    x[:k] = s[:k]
    x.setflags(write=False)
    return x


def n_structured(B, C=5):
    return len(structured_boards(B, C)[1])


def batch_indices(batch, B, C=5, seed=0, n_pool=None):
    """Which pool board sits at which index of a batch of `batch` boards: random pool boards, with the structured boards at
    index 0 .. 4, at 13 .. 21 (across the seam between the first two 16-board groups), over the whole last group (whole or
    ragged) of a batch of more than two groups, and on the last three indices. A batch of fewer than 8 boards starts with a
    float-plane board and alternates structured and random boards, so that a handful of boards is never structured boards only: on
    those half of a network's ReLUs are dead, and a defect behind a dead ReLU cannot be seen."""
    n_pool = n_pool or (POOL if B <= 9 else WIDE_POOL)
    ns = min(n_structured(B, C), n_pool)
    rs = np.random.RandomState(batch * 31 + B + 1009 * seed)
    m = rs.randint(ns, n_pool, size=batch)
    order = [2, 0, 3, 11, 7, 4, 8, 5, 6, 12, 9, 1, 10, 13]                      # full, empty, a corner, float planes, ...
    order = [o for o in order if o < ns]

    def place(start, ids):
        for j, s in enumerate(ids):
            if 0 <= start + j < batch:
                m[start + j] = s

    if batch < 8:
        m[:] = rs.randint(ns, 24, size=batch)          # (the defect catalogue evaluates its whole-forward defects on pool[:24])
        # the float-plane boards are the liveliest of the pool; in this order every tiny case sees every defect of the catalogue
        # of test_net_reference.py (a single weight sits behind a dead ReLU on about half of all single boards)
        m[0:6:2] = [ns - 2, ns - 3, ns - 1][:len(m[0:6:2])]
        m[1::2] = order[:len(m[1::2])]
        return m
    if batch > 32:
        place(batch - (batch % 16 or 16), order[4:] + order[:4])
    if batch >= 9:
        place(batch - 3, [order[3], order[5], order[0]])                          # ... ends on a corner stone and the full board
    if batch >= 22:
        place(13, order[5:] + order[:1])
    place(0, order[:5])
    return m


# ------------------------------------------------------------------------------------------------------------------
# 2. conditioned networks
# ------------------------------------------------------------------------------------------------------------------
def project_to_fp16_grid(sd):
    """Every 3x3 conv weight replaced by its fp16 rounding (as test_gpu_w16._grid_sd): the two-product kernels' networks."""
    out = dict(sd)
    for k, v in sd.items():
        if v.ndim == 4 and v.shape[2] == 3:
            out[k] = v.astype(np.float16).astype(np.float32)
    return out


def conditioned_state_dict(n_block, inplanes, planes, board_size, seed, grid=False, alpha=0.3):
    """A state_dict with make_state_dict's keys, deterministic from the arguments, on which a forward test can see an error:
      * the second BatchNorm of every block has its weight and bias scaled by `alpha`, so a block adds a fraction of its
        input's variance instead of doubling it and the tower's output stays O(1) at any depth (per-channel different
        weight, bias, mean and variance stay in every trunk BatchNorm: the fold is part of what is tested);
      * the BatchNorms of the two 1x1 head convs are centred and normalised on the float64 activations of a calibration
        batch (`pool(board_size, inplanes)`, which is also what the tests draw their batches from), then
        shifted by +0.3, so each head's ReLU passes a little more than half of its inputs;
      * value_fc1's bias is set per unit to minus the median of its input over the calibration batch plus a spread, so its
        ReLU passes about half;
      * policy_fc is scaled to logits of standard deviation 1.25 over the calibration batch (less, down to 1.05, where that
        keeps min p above 1e-7), value_fc2's weight to z of standard deviation 0.45 (less,
        down to 0.32, if |z| would pass 1.4), its bias to z of mean 0.
    grid=True: the 3x3 conv weights are projected onto the fp16 grid first (ao_net_products() == 2) and the calibration is
    done on the projected weights."""
    import torch
    import torch.nn.functional as F
    sd = pvnet_weights.make_state_dict(n_block, inplanes, planes, board_size, seed)
    if grid:
        sd = project_to_fp16_grid(sd)
    for i in range(n_block):
        sd["layers.%d.bn2.weight" % i] = sd["layers.%d.bn2.weight" % i] * np.float32(alpha)
        sd["layers.%d.bn2.bias" % i] = sd["layers.%d.bn2.bias" % i] * np.float32(alpha)
    xc = pool(board_size, inplanes)
    t = forward(sd, xc)["trunk"]
    for head, c in (("policy_head.policy_head", "policy_head.policy_bn"), ("value_head.value_head", "value_head.value_bn")):
        y = F.conv2d(t, torch.from_numpy(sd[head + ".weight"]).double())
        sd[c + ".running_mean"] = y.mean((0, 2, 3)).numpy().astype(np.float32)
        sd[c + ".running_var"] = (y.std((0, 2, 3)).numpy() ** 2).astype(np.float32)
        sd[c + ".weight"] = np.ones_like(sd[c + ".weight"])
        sd[c + ".bias"] = np.full_like(sd[c + ".bias"], 0.3)
    o = forward(sd, xc, trunk=t)
    pre = o["hv"] @ torch.from_numpy(sd["value_head.value_fc1.weight"]).double().T
    rs = np.random.RandomState(seed + 17)
    sd["value_head.value_fc1.bias"] = (-pre.median(dim=0).values.numpy() + 0.25 * pre.std().item() * rs.standard_normal(planes)).astype(np.float32)
    o = forward(sd, xc, trunk=t)
    lg = o["logits"]
    lo, hi = 1.05 / lg.std().item(), 1.25 / lg.std().item()

    def p_min(k):
        return torch.softmax(lg * k, dim=1).min().item()

    ks = hi
    if p_min(hi) < 1e-7:                                                      # (min p >= 1e-8 is the condition)
        for _ in range(20):
            ks = 0.5 * (lo + hi)
            lo, hi = (ks, hi) if p_min(ks) >= 1e-7 else (lo, ks)
        ks = lo
    sd["policy_head.policy_fc.weight"] = sd["policy_head.policy_fc.weight"] * np.float32(ks)
    sd["policy_head.policy_fc.bias"] = sd["policy_head.policy_fc.bias"] * np.float32(ks)
    zc = o["z"] - o["z"].mean()
    kz = max(min(0.45 / zc.std().item(), 1.4 / zc.abs().max().item()), 0.32 / zc.std().item())
    sd["value_head.value_fc2.weight"] = sd["value_head.value_fc2.weight"] * np.float32(kz)
    sd["value_head.value_fc2.bias"] = np.zeros_like(sd["value_head.value_fc2.bias"])
    o = forward(sd, xc, trunk=t)
    sd["value_head.value_fc2.bias"] = np.full_like(sd["value_head.value_fc2.bias"], -o["z"].mean().item())
    return sd


def conditioning_report(sd, x):
    """The figures the conditions of a test network are stated in, of the float64 reference on planes `x`."""
    import torch
    o = forward(sd, x)
    p = torch.softmax(o["logits"], dim=1)
    return dict(trunk_rms=o["trunk"].pow(2).mean().sqrt().item(), trunk_max=o["trunk"].abs().max().item(),
                logit_std=o["logits"].std().item() if o["logits"].numel() > 1 else 0.0, p_min=p.min().item(),
                z_absmax=o["z"].abs().max().item(), z_std=o["z"].std().item() if o["z"].numel() > 1 else 0.0,
                hp_live=(o["hp"] > 0).double().mean().item(), hv_live=(o["hv"] > 0).double().mean().item(),
                h1_live=(o["h1"] > 0).double().mean().item())


# ------------------------------------------------------------------------------------------------------------------
# references of a (network, pool) pair, computed once per process
# ------------------------------------------------------------------------------------------------------------------
# (nb, B, planes, C) -> added to the seed, C = 5 never: the networks of the input-plane cases that miss a condition of
# test_net_reference.py on the seed of their shape, and the figure the offset fixes
SEED_OFFSET = {
    (2, 9, 128, 9): 1,     # max |z| over the pool 1.69 against the limit of 1.5 (1.40 with the offset)
    (2, 9, 64, 7): 1,      # layers.1.bn1.running_var drew one value twice: 63 distinct of 64 (the fold must differ per channel)
    (1, 9, 256, 1): 2,     # centred logits of the 40-board batch: standard deviation 0.993 (0.925 at offset 1) against 1.0
}


def case_seed(nb, B, planes, C=5):
    return 100 + nb + 10 * B + planes + (SEED_OFFSET.get((nb, B, planes, C), 0) if C != 5 else 0)


@functools.lru_cache(maxsize=None)
def case_network(nb, B, planes, grid=False, C=5):
    return conditioned_state_dict(nb, C, planes, B, case_seed(nb, B, planes, C), grid=grid)


@functools.lru_cache(maxsize=None)
def pool_reference(nb, B, planes, grid=False, C=5):
    """(float64 reference, float32 reference) of case_network(...) on pool(B, C), as dicts of float64 numpy arrays
    `logits` (centred), `z`, `p`, `v`."""
    import torch
    sd = case_network(nb, B, planes, grid, C)
    x = pool(B, C)
    out = []
    for dt in (torch.float64, torch.float32):
        o = forward(sd, x, dt)
        lg = o["logits"].double()
        out.append(dict(logits=centred(lg).numpy(), z=o["z"].double().numpy(), p=torch.softmax(lg, dim=1).numpy(),
                        v=torch.tanh(o["z"].double()).numpy()))
    return tuple(out)


E32_FLOOR = 1e-6     # reading a logit back through an fp32 softmax and log (or z through tanh / atanh at |z| <= 1.5) costs a few
                     # ulp of 6e-8 times a condition number below 6; on the smallest networks E32 itself falls under that


def units(nb, B, planes, grid, boards, C=5):
    """(E32_l, E32_z) of a case: the float32-vs-float64 distance of the plain reference over the pool boards `boards` the
    case's batch is made of, each with the floor of 1e-6."""
    r64, r32 = pool_reference(nb, B, planes, grid, C)
    u = np.unique(boards)
    return (max(float(np.abs(r32["logits"][u] - r64["logits"][u]).max()), E32_FLOOR),
            max(float(np.abs(r32["z"][u] - r64["z"][u]).max()), E32_FLOOR))


def saturation_table():
    """The rows of the table in this module's docstring, from make_state_dict's weights (float64, CPU)."""
    import torch
    rows = []
    for nb, B, planes, batch in [(4, 9, 128, 70), (10, 9, 128, 33), (2, 15, 128, 40), (3, 9, 64, 32), (1, 3, 32, 5), (2, 7, 96, 64),
                                 (2, 7, 128, 20), (1, 3, 128, 3)]:
        sd = pvnet_weights.make_state_dict(nb, 5, planes, B, 100 + nb)
        rs = np.random.RandomState(batch)
        x = (rs.rand(batch, 5, B, B) < 0.3).astype(np.float32)
        x[:, 4] = (rs.rand(batch, 1, 1) < 0.5).astype(np.float32)
        o = forward(sd, x)
        p = torch.softmax(o["logits"], dim=1).numpy()
        v = torch.tanh(o["z"]).numpy()
        rows.append(dict(case=(nb, B, planes, batch), distinct_v=len(set(v.astype(np.float32))), one_minus_absv_min=float((1 - np.abs(v)).min()),
                         one_minus_absv_max=float((1 - np.abs(v)).max()), share_p_below_1e6=float((p < 1e-6).mean()),
                         median_max_p=float(np.median(p.max(axis=1))), hv_live=float((o["hv"] > 0).double().mean())))
    return rows


# ------------------------------------------------------------------------------------------------------------------
# 6. the cases of tests/test_gpu_net_precision.py: every kernel family, by name, at its seams
# ------------------------------------------------------------------------------------------------------------------
class Case:
    """One forward of the precision test: network (nb, B, planes; conv weights on the fp16 grid or not), batch size, trunk
    mode, the environment the Net is created under, the kernel the library must name, and the bound's multiplier."""

    def __init__(self, family, kernel, nb, B, batch, mode=0, planes=128, env=None, grid=False, products=None, what="", C=5):
        self.family, self.kernel, self.nb, self.B, self.batch, self.mode, self.planes = family, kernel, nb, B, batch, mode, planes
        self.C = C                                                                   # input planes of conv1
        self.env, self.grid, self.what = dict(env or {}), grid, what
        self.products = products if products is not None else (2 if grid else 3)     # what net.products() must answer
        # 4 x E32 for the kernels that are fp32 throughout: another summation order is worth about 2 x, and the CPU's own
        # order varies between machines by as much again. 16 x E32 for the split-fp16 families (named k_*h / k_*hk / k_*hb:
        # 128 planes, three- and two-product forms): activations held as two fp16 halves carry 22 bits against 24, a
        # further 4 x. The per-board path of a 128-plane network (mode 3) is k_conv_cells_h, a split-fp16 kernel: 16 x.
        self.mult = 16 if is_split_fp16(kernel) else 4
        env_id = "".join("-%s=%s" % (k[3:].lower(), v) for k, v in sorted(self.env.items()))
        self.id = "%s-nb%d-B%d-%s%d-m%d%s-%s%s" % (family, nb, B, "" if planes == 128 else "p%d-" % planes, batch, mode, env_id,
                                                   "w16grid" if grid else "w32", "" if C == 5 else "-C%d" % C)

    def net_key(self):
        return (self.nb, self.B, self.planes, self.grid, self.C)

    def boards(self):
        return batch_indices(self.batch, self.B, self.C)


def is_split_fp16(kernel):
    head = kernel.split("<")[0]
    return head in ("k_conv_cells_h", "k_conv_cells_h_w16", "k_row16hk", "k_row16hk_w16", "k_layer16hk", "k_layer16hk_w16", "k_layer16h",
                    "k_layer16h_w16", "k_trunk16h", "k_trunk16h_w16", "k_trunk16hb", "k_trunk16hb_w16", "k_boardh", "k_boardh_w16")


def _split_fp16_cases():
    out = []

    def both(family, kernel, nb, B, batch, mode=0, env=None, w16=True, what=""):
        """the three-product form on arbitrary fp32 weights, and -- where a _w16 form exists -- the two-product form on
        weights projected onto the fp16 grid (w16=False: the family has none, the grid network runs the same kernel)"""
        head, _, tail = kernel.partition("<")
        out.append(Case(family, kernel, nb, B, batch, mode, env=env, grid=False, what=what))
        out.append(Case(family, (head + "_w16<" + tail) if w16 else kernel, nb, B, batch, mode, env=env, grid=True, what=what))

    # a handful of boards: the per-board path (ao_net_forward's auto mode up to 2592 cells of 9x9, 5400 of wider boards)
    for nb, B, batch in [(4, 9, 1), (4, 9, 5), (4, 9, 32), (10, 9, 3), (2, 7, 20), (2, 15, 8)]:
        both("conv_cells_h", "k_conv_cells_h<%d, 8>" % B, nb, B, batch, what="per-board path")
    # k_row16hk: 1, 2 (mode 5: auto takes the per-board path there), 3 .. 47 groups of 16 boards
    for nb, B, batch, mode in [(4, 9, 9, 5), (4, 9, 16, 5), (4, 9, 31, 5), (10, 9, 33, 0), (4, 9, 750, 0), (10, 9, 752, 0), (2, 7, 100, 0)]:
        both("row16hk", "k_row16hk<%d>" % B, nb, B, batch, mode, what="%d groups" % ((batch + 15) // 16))
    # k_layer16hk<B, 4>: 48 .. 64 groups
    for nb, B, batch in [(4, 9, 760), (4, 9, 1024), (10, 9, 768), (10, 9, 1015), (2, 7, 1000)]:
        both("layer16hk4", "k_layer16hk<%d, 4>" % B, nb, B, batch, what="%d groups" % ((batch + 15) // 16))
    # k_layer16hk<B, 2>: the two-workgroup form, planned through AO_KSPLIT only; it has no two-product form
    for nb, B, batch in [(4, 9, 1040), (4, 9, 2048), (10, 9, 1999)]:
        both("layer16hk2", "k_layer16hk<%d, 2>" % B, nb, B, batch, env={"AO_KSPLIT": "48,64,128"}, w16=False,
             what="%d groups" % ((batch + 15) // 16))
    # k_layer16h: mode 6 at any batch size, and 65 .. 191 groups in auto mode
    for nb, B, batch, mode in [(4, 9, 70, 6), (4, 9, 1500, 6), (4, 9, 3100, 6), (10, 9, 33, 6), (4, 9, 1040, 0), (4, 9, 3056, 0),
                               (10, 9, 3050, 0), (2, 7, 2000, 0)]:
        both("layer16h", "k_layer16h<%d>" % B, nb, B, batch, mode, what="%d groups" % ((batch + 15) // 16))
    # the resident trunk on float planes (k_trunk16h; ao_search's k_trunk16hb differs in how conv1 reads its planes and is tied
    # to it by the equality tests of test_gpu_net.py): 192 groups exactly, a ragged 193rd, 4096 boards; both activation formats.
    # AO_TRUNK_FMT=1 has no two-product form.
    for nb, B, batch, fmt in [(4, 9, 3072, 0), (4, 9, 3073, 0), (4, 9, 4096, 0), (10, 9, 3073, 0), (10, 9, 4096, 0), (2, 7, 3104, 0),
                              (4, 9, 3072, 1), (4, 9, 3073, 1), (4, 9, 4096, 1), (10, 9, 4096, 1)]:
        both("trunk16h_fmt%d" % fmt, "k_trunk16h<%d, 4, %d>" % (B, fmt), nb, B, batch, env={"AO_TRUNK_FMT": str(fmt)}, w16=fmt == 0,
             what="%d groups" % ((batch + 15) // 16))
    # k_boardh: boards wider than 9 from 64 boards on; below, the per-layer kernel on column tiles
    for nb, B, batches in [(2, 10, (64, 65, 128)), (10, 11, (64, 129)), (2, 13, (65, 200)), (2, 15, (64, 65, 130)), (10, 15, (64, 256))]:
        for batch in batches:
            both("boardh", "k_boardh<%d, 1>" % B, nb, B, batch, what="one board per workgroup")
    for nb, B, batch, mode in [(2, 10, 63, 0), (10, 11, 63, 0), (2, 13, 63, 0), (2, 15, 63, 0), (10, 15, 40, 0), (2, 13, 33, 6)]:
        both("layer16h_wide", "k_layer16h<%d>" % B, nb, B, batch, mode, what="column tiles of a wide board")
    # the even board widths: every family is instantiated per width, and a row or column-tile seam that is wrong only at an
    # even width shows on none of the cases above. 4 / 6 / 8 walk the batch-size ladder of the narrow boards, 12 / 14 the two
    # kernels of the wide ones (ao_net_plan_kernel names these for 2 blocks of 128 planes)
    first = len(out)
    for B, ladder in [(4, [("conv_cells_h", "k_conv_cells_h<4, 8>", (5, 130)), ("row16hk", "k_row16hk<4>", (300,)),
                           ("layer16hk4", "k_layer16hk<4, 4>", (1000,)), ("layer16h", "k_layer16h<4>", (2000,)),
                           ("trunk16h_fmt0", "k_trunk16h<4, 4, 0>", (3073,))]),
                      (6, [("conv_cells_h", "k_conv_cells_h<6, 8>", (65,)), ("row16hk", "k_row16hk<6>", (130,)),
                           ("layer16hk4", "k_layer16hk<6, 4>", (1024,)), ("trunk16h_fmt0", "k_trunk16h<6, 4, 0>", (3073,))]),
                      (8, [("conv_cells_h", "k_conv_cells_h<8, 8>", (40,)), ("row16hk", "k_row16hk<8>", (61, 300)),
                           ("layer16hk4", "k_layer16hk<8, 4>", (1000,)), ("layer16h", "k_layer16h<8>", (2000,)),
                           ("trunk16h_fmt0", "k_trunk16h<8, 4, 0>", (4096,))]),
                      (12, [("conv_cells_h", "k_conv_cells_h<12, 8>", (5,)), ("layer16h_wide", "k_layer16h<12>", (63,)),
                            ("boardh", "k_boardh<12, 1>", (64, 65, 130))]),
                      (14, [("conv_cells_h", "k_conv_cells_h<14, 8>", (5,)), ("layer16h_wide", "k_layer16h<14>", (63,)),
                            ("boardh", "k_boardh<14, 1>", (64, 65, 130))])]:
        for family, kernel, batches in ladder:
            for batch in batches:
                both(family, kernel, 2, B, batch, env={"AO_TRUNK_FMT": "0"} if family == "trunk16h_fmt0" else None,
                     what="even width %d" % B)
    out[first:] = sorted(out[first:], key=lambda c: (c.B, c.grid))       # (stable: the cases of one network stay together)
    return out


def _fp32_cases():
    out = []
    # modes 1 .. 4 on the shapes of test_gpu_net.test_forward_vs_torch_fp32
    for nb, B, planes, batch in [(4, 9, 128, 70), (10, 9, 128, 33), (2, 15, 128, 40), (3, 9, 64, 32), (1, 3, 32, 5), (2, 7, 96, 64),
                                 (2, 7, 128, 20), (1, 3, 128, 3)]:
        cells = "k_conv_cells_h<%d, 8>" % B if planes == 128 else "k_conv_cells<%d>" % B
        for mode, family, kernel in [(1, "conv3x3", "k_conv3x3<%d>" % B), (2, "trunk16", "k_trunk16<%d>" % B),
                                     (3, cells.split("<")[0][2:], cells), (4, "layer16", "k_layer16<%d>" % B)]:
            out.append(Case(family, kernel, nb, B, batch, mode, planes=planes, what="mode %d" % mode))
    # ... and at two even widths (a wide board and a narrow one), as (2, 7, 128, 20) and (2, 15, 128, 40) do for 7 and 15
    # (batches of 20 boards, but 21 on 8x8: the 20 boards batch_indices draws there have z of standard deviation 0.22, under
    # the 0.3 that test_net_reference.py asks of a batch; likewise 61 boards for k_row16hk<8> above, where 63 give 0.297)
    for B, batch in ((12, 20), (8, 21)):
        for mode, family, kernel in [(1, "conv3x3", "k_conv3x3<%d>" % B), (2, "trunk16", "k_trunk16<%d>" % B),
                                     (3, "conv_cells_h", "k_conv_cells_h<%d, 8>" % B), (4, "layer16", "k_layer16<%d>" % B)]:
            out.append(Case(family, kernel, 2, B, batch, mode, what="mode %d, even width" % mode))
    # 160 .. 512 planes: the fp32-MFMA layer kernels whatever the mode; widths that are exported zero-padded (100 -> 128 runs
    # on the split-fp16 kernels, 200 -> 224 and 300 -> 320 on k_layer16)
    for nb, B, planes, batch in [(2, 9, 256, 40), (1, 7, 192, 700), (2, 15, 160, 70), (3, 9, 224, 1024), (1, 9, 512, 600), (2, 13, 384, 20),
                                 (1, 3, 512, 3), (2, 9, 200, 64), (1, 9, 300, 48)]:
        out.append(Case("layer16_wide", "k_layer16<%d>" % B, nb, B, batch, 0, planes=planes, what="%d planes" % planes))
    out.append(Case("row16hk_padded", "k_row16hk<9>", 2, 9, 300, 0, planes=100, what="100 planes zero-padded to 128"))
    out.append(Case("boardh_padded", "k_boardh<15, 1>", 2, 15, 70, 0, planes=100, what="100 planes zero-padded to 128"))
    return out


INPLANES = (1, 3, 4, 7, 8, 9, 12)       # a single ragged quad (1, 3), a quad exactly full (4, 8, 12), two quads with bit 6 / bit 7 of
                                        # the plane byte in use (7, 8), three quads (9, 12: nchq32 goes from 2 to 4)
INPLANES_W16 = (3, 8, 9, 12)            # the two-product kernels have a conv1 text of their own; the packing is shared


def _inplanes_cases():
    """Every conv1 form at input-plane counts other than 5 (every case above runs 5): conv1 is the one layer whose packing
    and kernel text depend on that number. One case per C and form, at the smallest shape that reaches the form; 2 blocks
    but for the 256-plane network."""
    out = []
    for C in INPLANES:
        # fp32 throughout: the three packings of ao_net_finalize (nchq32 / nchq16 / nchq1) and cq0_real of the resident trunk
        for mode, family, kernel in [(1, "conv3x3", "k_conv3x3<9>"), (2, "trunk16", "k_trunk16<9>"), (3, "conv_cells", "k_conv_cells<9>"),
                                     (4, "layer16", "k_layer16<9>")]:
            out.append(Case(family, kernel, 2, 9, 33, mode, planes=64, what="mode %d, %d input planes" % (mode, C), C=C))
        out.append(Case("layer16_wide", "k_layer16<9>", 1, 9, 40, 0, planes=256, what="256 planes, %d input planes" % C, C=C))
        # split fp16: conv1's hi / lo packing, zero-padded to one 32-channel block
        # (7 boards at C = 3, not 5: on the five boards batch_indices draws there, unit 0 of value_fc1 is dead in the float64
        # reference, and the catalogue's "value_fc1: row 0 zeroed" moves nothing)
        nine = [("conv_cells_h", "k_conv_cells_h<9, 8>", 7 if C == 3 else 5, 0, None), ("row16hk", "k_row16hk<9>", 33, 0, None),
                ("layer16hk4", "k_layer16hk<9, 4>", 760, 0, None), ("layer16h", "k_layer16h<9>", 70, 6, None),
                ("trunk16h_fmt0", "k_trunk16h<9, 4, 0>", 3073, 0, {"AO_TRUNK_FMT": "0"})]
        wide = [("boardh", "k_boardh<15, 1>", 65, 0, None), ("layer16h_wide", "k_layer16h<15>", 63, 0, None)]
        for B, forms in ((9, nine), (15, wide)):
            for family, kernel, batch, mode, env in forms:
                out.append(Case(family, kernel, 2, B, batch, mode, env=env, what="%d input planes" % C, C=C))
        if C in INPLANES_W16:
            for B, forms in ((9, nine), (15, wide[:1])):
                for family, kernel, batch, mode, env in forms:
                    head, _, tail = kernel.partition("<")
                    out.append(Case(family, head + "_w16<" + tail, 2, B, batch, mode, env=env, grid=True, what="%d input planes" % C, C=C))
    return out


CASES = _split_fp16_cases() + _fp32_cases() + _inplanes_cases()
