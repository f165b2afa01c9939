"""Networks and references of the fp16-forward tests (tests/test_fp16_forward_host.py on the CPU, tests/test_gpu_fp16_forward.py
on the GPU).

"fp16 forward" (ao_net_precision, include/omok_hip.h) is, on the host,

    net_reference.forward(project_to_fp16_grid(sd), x, act_round=r16),    r16(t) = clamp(t, max=65504).half().to(t.dtype)

on planes x that are fp16 numbers: fp16 conv weights, every stored trunk activation rounded once to fp16 (to nearest even),
everything else exact. Two networks make a test of the one-product kernels sharp:

  * the EXACT network (`exact_network`): conv weights in {-1, 0, 1}, trunk BatchNorms that fold to {0.5, 1} x integers, so that
    every activation the float64 reference stores IS an fp16 number. Rounding changes nothing there: the fp16 forward must return
    the bits of the default forward -- and any dropped tap, wrong residual source, wrong handed row or stale low fragment shows;
  * its PERTURBED twin (`perturbed_pair`): 32 channels of conv1's BatchNorm and of every block's first BatchNorm scaled by
    1 +- 2^-12. Their activations then sit 2^-12 (relative) off an fp16 number: rounding to NEAREST takes them back exactly, so
    the fp16 forward of the twin equals the default forward of the unperturbed network bit for bit, while the default forward of
    the twin (which keeps the low halves) differs. Truncation, or a kernel that silently kept its low halves, fails.
"""
import functools

import numpy as np

import net_reference as nr
import pvnet_weights

SEED = 11


def r16(t):
    import torch
    return torch.clamp(t, max=65504.0).to(torch.float16).to(t.dtype)


def trunk_bns(nb):
    return ["bn1"] + ["layers.%d.bn%d" % (i, j) for i in range(nb) for j in (1, 2)]


def binary_pool(B):
    """The 0/1 boards of net_reference.pool(B) (its float-plane boards left out), read-only."""
    x = nr.pool(B)
    keep = np.all((x == 0) | (x == 1), axis=(1, 2, 3))
    out = np.ascontiguousarray(x[keep])
    out.setflags(write=False)
    return out


def as_folded(sd):
    """`sd` with the trunk BatchNorms' running_var as the float64 1 - 1e-5: what the library's fold (w / sqrt(var + 1e-5) in double,
    cast to float) makes of the float32 value is then exactly what the float64 reference computes."""
    out = dict(sd)
    for n in trunk_bns(nr.n_blocks(sd)):
        out[n + ".running_var"] = np.full(sd[n + ".running_var"].shape, 1.0 - 1e-5, np.float64)
    return out


def fold_is_exact(sd):
    """The library's fold of every trunk BatchNorm (scale s = w / sqrt(var + 1e-5) in double, cast to float; shift b - mean * s in
    double, cast to float) returns the weight itself and the exact shift b - mean * w. The double s is NOT w (the float32 nearest
    to 1 - 1e-5 is 6.8e-9 off), so a shift whose exact value is 0 with mean != 0 would come out as -+6.8e-9: a positive
    activation of that size is no fp16 number (it rounds to 0), and a kernel that hands its last layer to the heads in fp32
    registers (k_boardh) would show it where one that stores two halves does not. exact_network draws no such channel."""
    for n in trunk_bns(nr.n_blocks(sd)):
        w, b, m = (sd[n + k].astype(np.float64) for k in (".weight", ".bias", ".running_mean"))
        s = w / np.sqrt(sd[n + ".running_var"].astype(np.float64) + 1e-5)
        if not (s.astype(np.float32) == sd[n + ".weight"]).all() or not ((b - m * s).astype(np.float32).astype(np.float64) == b - m * w).all():
            return False
    return True


def calibrate_heads(sd, xc, seed):
    """The head calibration of net_reference.conditioned_state_dict on the float64 trunk of `sd` over the boards `xc`: head
    BatchNorms centred, value_fc1's bias at the median, policy_fc scaled to logits of standard deviation <= 1.25 with
    min p >= 1e-7, value_fc2 scaled to |z| <= 1.4 -- so that a search on the network has usable priors."""
    import torch
    import torch.nn.functional as F
    planes = sd["conv1.weight"].shape[0]
    t = nr.forward(as_folded(sd), xc)["trunk"]
    for head, c in (("policy_head.policy_head", "policy_head.policy_bn"), ("value_head.value_head", "value_head.value_bn")):
        y = F.conv2d(t, torch.from_numpy(sd[head + ".weight"]).double())
        sd[c + ".running_mean"] = y.mean((0, 2, 3)).numpy().astype(np.float32)
        sd[c + ".running_var"] = (y.std((0, 2, 3)).numpy() ** 2).astype(np.float32)
        sd[c + ".weight"] = np.ones_like(sd[c + ".weight"])
        sd[c + ".bias"] = np.full_like(sd[c + ".bias"], 0.3)
    o = nr.forward(sd, xc, trunk=t)
    pre = o["hv"] @ torch.from_numpy(sd["value_head.value_fc1.weight"]).double().T
    rs = np.random.RandomState(seed + 17)
    sd["value_head.value_fc1.bias"] = (-pre.median(dim=0).values.numpy() + 0.25 * pre.std().item() * rs.standard_normal(planes)).astype(np.float32)
    o = nr.forward(sd, xc, trunk=t)
    lg = o["logits"]
    lo, hi = 1.05 / lg.std().item(), 1.25 / lg.std().item()

    def p_min(k):
        return torch.softmax(lg * k, dim=1).min().item()

    ks = hi
    if p_min(hi) < 1e-7:
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
    o = nr.forward(sd, xc, trunk=t)
    sd["value_head.value_fc2.bias"] = np.full_like(sd["value_head.value_fc2.bias"], -o["z"].mean().item())
    return sd


@functools.lru_cache(maxsize=None)
def exact_network(nb, B, seed=SEED):
    """The exact network of (nb blocks, board B), 5 input planes, 128 planes; heads calibrated on binary_pool(B). Read-only."""
    sd = pvnet_weights.make_state_dict(nb, 5, 128, B, seed)
    rs = np.random.RandomState(seed + 5)
    for k in list(sd):
        v = sd[k]
        if v.ndim == 4 and v.shape[2] == 3:
            d = 0.5 if k == "conv1.weight" else 0.01
            sd[k] = (np.sign(rs.standard_normal(v.shape)) * (rs.rand(*v.shape) < d)).astype(np.float32)
    for n in trunk_bns(nb):
        sd[n + ".weight"] = rs.choice([0.5, 1.0] if n in ("bn1", "layers.0.bn1") else [1.0, 1.0], 128).astype(np.float32)
        sd[n + ".running_var"] = np.full(128, np.float32(1 - 1e-5), np.float32)
        sd[n + ".running_mean"] = rs.randint(-1, 2, 128).astype(np.float32)
        sd[n + ".bias"] = rs.randint(-1, 2, 128).astype(np.float32)
        # (the shift b - mean * w must not be an exact 0 on a channel with mean != 0: see fold_is_exact)
        clash = (sd[n + ".running_mean"] != 0) & (sd[n + ".bias"] == sd[n + ".running_mean"] * sd[n + ".weight"])
        sd[n + ".bias"][clash] = 0
    return calibrate_heads(sd, binary_pool(B), seed)


@functools.lru_cache(maxsize=None)
def perturbed_pair(nb, B, seed=SEED):
    """(twin, perturbed): the exact network with mean and bias zeroed on 32 channels of bn1 and of every layers.i.bn1, and the same
    network with those channels' weights multiplied by 1 + 2^-12 (16 of them) and 1 - 2^-12 (the other 16)."""
    twin, pert = dict(exact_network(nb, B, seed)), dict(exact_network(nb, B, seed))
    rs = np.random.RandomState(3)
    for n in ["bn1"] + ["layers.%d.bn1" % i for i in range(nb)]:
        w, m, b = twin[n + ".weight"].copy(), twin[n + ".running_mean"].copy(), twin[n + ".bias"].copy()
        ch = rs.permutation(128)[:32]
        w[ch[:16]] *= np.float32(1 + 2.0 ** -12)
        w[ch[16:]] *= np.float32(1 - 2.0 ** -12)
        m[ch] = 0
        b[ch] = 0
        twin[n + ".running_mean"], twin[n + ".bias"] = m, b
        pert[n + ".weight"], pert[n + ".running_mean"], pert[n + ".bias"] = w, m, b
    return twin, pert


def spy_forward(sd, x):
    """(float64 reference of as_folded(sd) on x, the activations it stored between trunk layers)."""
    acts = []

    def spy(t):
        acts.append(t.clone())
        return t

    return nr.forward(as_folded(sd), x, act_round=spy), acts


@functools.lru_cache(maxsize=None)
def exact_reference(nb, B):
    """(p [n, A], v [n]) float64 of the exact network on binary_pool(B)."""
    import torch
    o = nr.forward(as_folded(exact_network(nb, B)), binary_pool(B))
    return torch.softmax(o["logits"], dim=1).numpy(), torch.tanh(o["z"]).numpy()


def batch_of(B, batch, seed=0):
    """Indices into binary_pool(B) of a batch of `batch` boards: net_reference.batch_indices' placement of the structured boards at
    the seams, restricted to the 0/1 boards (a float-plane board is replaced by a random 0/1 board)."""
    x = nr.pool(B)
    keep = np.all((x == 0) | (x == 1), axis=(1, 2, 3))
    new_index = np.cumsum(keep) - 1
    m = nr.batch_indices(batch, B, seed=seed)
    rs = np.random.RandomState(batch + 7 * B + seed)
    repl = rs.choice(np.nonzero(keep)[0], size=batch)
    m = np.where(keep[m], m, repl)
    return new_index[m]
