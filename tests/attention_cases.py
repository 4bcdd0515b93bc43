"""Inputs, references and tolerances shared by the attention tests: the CPU
test of the references themselves (tests/test_attention_ref_cpu.py) and the
GPU tests of src/ops/attention.hip (tests/test_attention_gpu.py) build the
same cases here, on the CPU generator, so both see the same data.

Tolerances.  Every bound in TOL is 3 x the worst error of `emulated` (an fp32
PyTorch model of what a correct bf16 flash kernel may lose) against `ref64`
(fp64 on the same bf16 inputs), taken over all cases of its group and rounded
up to one significant digit.  The factor 3 covers what the emulation does not
model: hardware exp2 / log2 / reciprocal, the tile order of accumulation and
the split fp32 partial sums of dK / dV.  o, dq, dk, dv: worst per-row relative
L2 error (row_rel_err) and, as "q90", the 0.9 quantile of the per-row errors;
lse2, delta: worst absolute error.  None of these numbers came from a kernel's
output; tests/test_attention_ref_cpu.py measures them again, prints them
(pytest -s) and holds TOL to them.

Emulation vs fp64, as measured on the CPU (group, case B x S x H x KV):

   case                       o        o q90    dq       dq q90   dk       dk q90   dv       dv q90   lse2     delta
   grouped 1x256x8x8          2.85e-03 2.43e-03 2.15e-02 2.83e-03 4.68e-03 2.83e-03 3.99e-03 2.68e-03 8.14e-07 2.85e-02
   grouped 2x256x8x4          3.12e-03 2.44e-03 3.51e-02 2.86e-03 5.26e-03 2.73e-03 3.68e-03 2.67e-03 8.41e-07 3.46e-02
   grouped 1x384x32x8         3.04e-03 2.46e-03 1.07e-01 2.80e-03 4.31e-03 2.67e-03 3.19e-03 2.62e-03 8.96e-07 4.04e-02
   grouped 3x128x16x8         2.93e-03 2.41e-03 2.91e-01 2.98e-03 5.31e-03 2.83e-03 3.90e-03 2.70e-03 8.41e-07 3.55e-02
   grouped 1x128x16x16        3.08e-03 2.41e-03 9.82e-02 2.92e-03 7.37e-03 2.87e-03 3.83e-03 2.75e-03 7.06e-07 3.37e-02
   grouped 1x512x8x8          3.08e-03 2.47e-03 9.92e-03 2.77e-03 6.69e-03 2.73e-03 3.72e-03 2.69e-03 9.14e-07 2.97e-02
   grouped 3x256x6x2          3.03e-03 2.45e-03 3.01e-01 2.83e-03 3.82e-03 2.69e-03 3.64e-03 2.65e-03 8.52e-07 5.38e-02
   grouped worst              3.12e-03 2.47e-03 3.01e-01 2.98e-03 7.37e-03 2.87e-03 3.99e-03 2.75e-03 9.14e-07 5.38e-02
   grouped bound              1e-02    8e-03    1e+00    9e-03    3e-02    9e-03    2e-02    9e-03    3e-06    2e-01
   reference 1x128x1x1        2.68e-03 2.43e-03 5.18e-03 2.86e-03 3.84e-03 2.79e-03 3.09e-03 2.68e-03 5.74e-07 2.26e-02
   reference 1x256x4x2        2.94e-03 2.44e-03 1.72e-02 2.90e-03 3.62e-03 2.77e-03 3.71e-03 2.66e-03 7.98e-07 2.52e-02
   reference 2x512x8x2        3.10e-03 2.50e-03 2.41e-02 2.78e-03 5.17e-03 2.69e-03 3.61e-03 2.64e-03 9.04e-07 5.34e-02
   reference 1x384x4x4        2.93e-03 2.47e-03 1.07e-01 2.78e-03 5.52e-03 2.77e-03 3.87e-03 2.70e-03 8.04e-07 3.23e-02
   reference worst            3.10e-03 2.50e-03 1.07e-01 2.90e-03 5.52e-03 2.79e-03 3.87e-03 2.70e-03 9.04e-07 5.34e-02
   reference bound            1e-02    8e-03    4e-01    9e-03    2e-02    9e-03    2e-02    9e-03    3e-06    2e-01
   peaky 1x512x4x1 (scale 4)  2.64e-03 1.90e-03    -        -        -        -        -        -     2.39e-05    -
   peaky bound                8e-03    6e-03       -        -        -        -        -        -     8e-05       -
   sm_scale 0.03 1x256x4x2    2.86e-03 2.43e-03 2.08e-02 2.86e-03 3.49e-03 2.76e-03 3.38e-03 2.72e-03 9.49e-07 2.71e-02
   sm_scale 0.25 1x256x4x2    3.03e-03 2.45e-03 8.17e-02 2.82e-03 4.40e-03 2.79e-03 3.07e-03 2.65e-03 8.14e-07 3.68e-02
   sm_scale worst             3.03e-03 2.45e-03 8.17e-02 2.86e-03 4.40e-03 2.79e-03 3.38e-03 2.72e-03 9.49e-07 3.68e-02
   sm_scale bound             1e-02    8e-03    3e-01    9e-03    2e-02    9e-03    2e-02    9e-03    3e-06    2e-01
   ramp slope +3              2.82e-03 2.48e-03 5.85e-02 1.80e-02 1.47e-02 5.72e-03 3.61e-03 2.58e-03 2.38e-06 1.97e-02
   ramp slope +7              2.93e-03 2.54e-03 1.81e-01 4.61e-02 1.84e-02 5.92e-03 3.28e-03 2.70e-03 5.29e-06 1.76e-02
   ramp slope -3              2.87e-03 2.49e-03 7.72e-02 1.54e-02 9.54e-03 4.49e-03 3.23e-03 2.58e-03 1.57e-06 2.63e-02
   ramp worst                 2.93e-03 2.54e-03 1.81e-01 4.61e-02 1.84e-02 5.92e-03 3.61e-03 2.70e-03 5.29e-06 2.63e-02
   ramp bound                 9e-03    8e-03    6e-01    2e-01    6e-02    2e-02    2e-02    9e-03    2e-05    8e-02

The worst dQ row is always one of the first rows of a head: with two or three
keys and a nearly one-hot softmax, dZ = P (dP - delta) cancels down to the
rounding of the bf16 O inside delta.  That is the algorithm, the emulation shows
it, and so the worst-row bound of dQ is loose; the q90 bound is what holds the
other rows of dQ as tight as o, dK and dV.

The uniform-score bounds (UNIFORM_*) are derived, not measured: see there.
"""
import math
from collections import namedtuple

import torch

HD = 128
LOG2E = 1.4426950408889634
DEFAULT_SCALE = HD ** -0.5
QUANTITIES = ("o", "dq", "dk", "dv", "lse2", "delta")
FWD_QUANTITIES = ("o", "lse2")
ROW_QUANTITIES = ("o", "dq", "dk", "dv")


# ----------------------------------------------------------------- references
def _expand(x, G):
    # [B, S, KV, D] -> [B, H, S, D], query head h reads kv head h // G
    return x.transpose(1, 2).repeat_interleave(G, dim=1)


def _causal(S, device):
    return torch.ones(S, S, device=device, dtype=torch.bool).triu(1)


def ref64(q, k, v, sm_scale):
    """Materialised causal GQA softmax attention in float64 on the given
    (bf16) inputs, token-major like the kernels: q [B,S,H,D], k/v [B,S,KV,D].
    Returns o [B,S,H,D] and lse2 [B,H,S], the base-2 log-sum-exp of the scaled
    scores.  Differentiable: pass float64 leaves to get gradients."""
    B, S, H, D = q.shape
    G = H // k.shape[2]
    qd, kd, vd = q.double().transpose(1, 2), _expand(k.double(), G), _expand(v.double(), G)
    z = (qd @ kd.transpose(-1, -2)) * sm_scale
    z = z.masked_fill(_causal(S, q.device), float("-inf"))
    o = (z.softmax(-1) @ vd).transpose(1, 2)
    return o, torch.logsumexp(z, -1) * LOG2E


def ref64_all(q, k, v, do, sm_scale):
    """ref64 plus fp64 autograd: {o, lse2, delta, dq, dk, dv}."""
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o, lse2 = ref64(qd, kd, vd, sm_scale)
    dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), do.double())
    o = o.detach()
    delta = (do.double() * o).sum(-1).transpose(1, 2)  # [B, H, S]
    return dict(o=o, lse2=lse2.detach(), delta=delta, dq=dq, dk=dk, dv=dv)


def _bf(x):
    return x.bfloat16().float()


def emulated(q, k, v, sm_scale, do=None):
    """What a correct bf16 flash kernel may lose, in fp32 PyTorch: fp32 scores,
    P rounded to bf16 before P V (the row sum stays fp32), output rounded to
    bf16; backward with P and dZ rounded to bf16 before their products and the
    results rounded to bf16.  It sizes the tolerances and is no copy of the
    kernel's tiling.  Returns {o, lse2} and, given dO, {delta, dq, dk, dv}."""
    B, S, H, D = q.shape
    KV = k.shape[2]
    G = H // KV
    c = sm_scale * LOG2E
    qf, kf, vf = q.float().transpose(1, 2), _expand(k.float(), G), _expand(v.float(), G)
    mask = _causal(S, q.device)
    z2 = ((qf @ kf.transpose(-1, -2)) * c).masked_fill(mask, float("-inf"))
    m = z2.amax(-1, keepdim=True)
    p = torch.exp2(z2 - m)
    l = p.sum(-1, keepdim=True)
    o = ((_bf(p) @ vf) / l).transpose(1, 2).bfloat16()
    lse2 = (m + torch.log2(l)).squeeze(-1)
    out = dict(o=o, lse2=lse2)
    if do is None:
        return out
    dof = do.float().transpose(1, 2)                         # [B, H, S, D]
    delta = (dof * o.float().transpose(1, 2)).sum(-1)        # [B, H, S]
    P = torch.exp2(z2 - lse2.unsqueeze(-1))                  # masked entries: exp2(-inf) = 0
    dZ = P * (dof @ vf.transpose(-1, -2) - delta.unsqueeze(-1))
    Pb, dZb = _bf(P), _bf(dZ)
    dq = ((dZb @ kf) * sm_scale).transpose(1, 2).bfloat16()
    dk = (dZb.transpose(-1, -2) @ qf).view(B, KV, G, S, D).sum(2) * sm_scale
    dv = (Pb.transpose(-1, -2) @ dof).view(B, KV, G, S, D).sum(2)
    out.update(delta=delta, dq=dq, dk=dk.transpose(1, 2).bfloat16(), dv=dv.transpose(1, 2).bfloat16())
    return out


def row_rel_err(got, ref, floor_frac=0.05):
    """Per-row relative L2 error over the last dim, a row being one
    (b, s, head): |got - ref| / max(|ref|, floor_frac * median row norm of ref).
    Returns (errors [B, S, heads], share of rows whose denominator was the
    floor).  (Row 0 of dQ is exactly zero, hence the floor.)"""
    got, ref = got.double(), ref.double()
    n = ref.norm(dim=-1)
    floor = floor_frac * n.median()
    return (got - ref).norm(dim=-1) / n.clamp_min(floor), (n < floor).double().mean().item()


def errors(got, ref):
    """What the tests bound, for the quantities that `got` holds: the worst
    per-row relative error of o / dq / dk / dv under the quantity's name, the
    0.9 quantile of the per-row errors under name + "_q90", the worst absolute
    error of lse2 / delta."""
    out = {}
    for name in QUANTITIES:
        if name not in got:
            continue
        if name in ROW_QUANTITIES:
            e = row_rel_err(got[name], ref[name])[0].flatten()
            out[name] = e.max().item()
            out[name + "_q90"] = e.quantile(0.9).item()
        else:
            out[name] = (got[name].double() - ref[name].double()).abs().max().item()
    return out


def floored_share(ref):
    """{quantity: share of rows of the reference under row_rel_err's floor}."""
    return {n: row_rel_err(ref[n], ref[n])[1] for n in ROW_QUANTITIES if n in ref}


# --------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def random_inputs(B, S, H, KV, seed, scale=1.0):
    """q, k ~ scale * N(0, 1), v, dO ~ N(0, 1), rounded to bf16."""
    g = _gen(seed)
    q = (scale * torch.randn(B, S, H, HD, generator=g)).bfloat16()
    k = (scale * torch.randn(B, S, KV, HD, generator=g)).bfloat16()
    v = torch.randn(B, S, KV, HD, generator=g).bfloat16()
    do = torch.randn(B, S, H, HD, generator=g).bfloat16()
    return q, k, v, do


RAMP_A = 8.0       # |q| along u
RAMP_NOISE = 0.25  # std of the components of q and k orthogonal to u


def ramp_inputs(S, slope, seed=0):
    """B 1, H 2, KV 1, default sm_scale.  k[j] = g(j) u + noise with a fixed unit
    vector u (64 entries of +-1/8), q[i] = a u + noise, the noise in the 64
    dims where u is zero (it moves a score by ~0.06 log2 units).  Head 0 has
    a = RAMP_A and g such that the scaled base-2 score of key j is
    slope * j / 64: it rises by `slope` log2 units per 64-key tile.  Head 1 has
    a = -RAMP_A / 2, i.e. the slope -slope / 2: with one head alone and a
    negative slope, dK / dV of the late keys would decay by 2^(slope * j / 64)
    and most of their rows would sit under row_rel_err's floor."""
    g = _gen(1000 + seed + int(10 * abs(slope)))
    u = torch.zeros(HD)
    u[:64] = (torch.randint(0, 2, (64,), generator=g).float() * 2 - 1) / 8
    noise = torch.zeros(HD)
    noise[64:] = RAMP_NOISE
    c = DEFAULT_SCALE * LOG2E
    gj = slope * torch.arange(S, dtype=torch.float32) / 64 / (c * RAMP_A)
    k = gj[:, None] * u + noise * torch.randn(S, HD, generator=g)
    a = torch.tensor([RAMP_A, -RAMP_A / 2])
    q = a[None, :, None] * u + noise * torch.randn(S, 2, HD, generator=g)
    v = torch.randn(S, HD, generator=g)
    do = torch.randn(S, 2, HD, generator=g)
    return (q.view(1, S, 2, HD).bfloat16(), k.view(1, S, 1, HD).bfloat16(),
            v.view(1, S, 1, HD).bfloat16(), do.view(1, S, 2, HD).bfloat16())


def uniform_inputs(B, S, H, KV, seed):
    """q = k = 0 and v small integers in [-4, 4] (exact in bf16, fp32 sums of
    them exact): every score is 0, so o[s] = mean(v[0..s]), lse2[s] = log2(s+1)."""
    g = _gen(seed)
    q = torch.zeros(B, S, H, HD, dtype=torch.bfloat16)
    k = torch.zeros(B, S, KV, HD, dtype=torch.bfloat16)
    v = torch.randint(-4, 5, (B, S, KV, HD), generator=g).bfloat16()
    return q, k, v


def uniform_expected(v, H):
    """(o [B,S,H,D], lse2 [B,H,S]) in fp64 for uniform_inputs."""
    B, S, KV, D = v.shape
    n = torch.arange(1, S + 1, dtype=torch.float64, device=v.device)
    mean = v.double().cumsum(1) / n[None, :, None, None]
    o = mean.repeat_interleave(H // KV, dim=2)
    return o, torch.log2(n).expand(B, H, S)


# ---------------------------------------------------------------------- cases
Case = namedtuple("Case", "id group kind shape seed scale sm_scale backward")


def _rand(group, B, S, H, KV, seed, scale=1.0, sm_scale=DEFAULT_SCALE, tag="", backward=True):
    return Case(f"{tag}{B}x{S}x{H}x{KV}", group, "random", (B, S, H, KV), seed, scale, sm_scale, backward)


# (B*KV) % 8 == 0: the XCD-grouped work-group order of all three kernels;
# the last one is the head-major fallback with B > 1 and G = 3
GROUPED = [
    _rand("grouped", 1, 256, 8, 8, 11),      # G 1, one group per XCD
    _rand("grouped", 2, 256, 8, 4, 12),      # batch index > 0 inside the grouped map, G 2
    _rand("grouped", 1, 384, 32, 8, 13),     # G 4, odd number of key blocks, 128-row last forward block
    _rand("grouped", 3, 128, 16, 8, 14),     # 3 groups per XCD
    _rand("grouped", 1, 128, 16, 16, 15),    # 2 groups per XCD, one key block
    _rand("grouped", 1, 512, 8, 8, 16),      # two dK/dV workgroups per group, no middle block
    _rand("grouped", 3, 256, 6, 2, 17),      # fallback order, B > 1, G 3
]
# the shapes of the max-abs tests, and their peaky case: forward only, like the
# max-abs test of it (with logits this large the softmax is nearly one-hot and
# a quarter of the dQ rows are zero to within the floor)
REFERENCE = [
    _rand("reference", 1, 128, 1, 1, 21),
    _rand("reference", 1, 256, 4, 2, 22),
    _rand("reference", 2, 512, 8, 2, 23),
    _rand("reference", 1, 384, 4, 4, 24),
]
PEAKY = [_rand("peaky", 1, 512, 4, 1, 25, scale=4.0, backward=False)]
# input scale chosen so that the scaled scores keep the spread they have at the
# default (sm_scale * scale^2 = 128^-0.5): at scale 1 and sm_scale 0.25 some
# keys get no weight at all and 5 % of the dV rows sit under the floor
SM_SCALES = [
    _rand("sm_scale", 1, 256, 4, 2, 31, scale=(DEFAULT_SCALE / 0.03) ** 0.5, sm_scale=0.03, tag="s0.03_"),
    _rand("sm_scale", 1, 256, 4, 2, 32, scale=(DEFAULT_SCALE / 0.25) ** 0.5, sm_scale=0.25, tag="s0.25_"),
]
RAMP_S = 512
RAMPS = [Case(f"slope{sl:+d}", "ramp", "ramp", (1, RAMP_S, 2, 1), 0, sl, DEFAULT_SCALE, True) for sl in (3, 7, -3)]
ALL_CASES = GROUPED + REFERENCE + PEAKY + SM_SCALES + RAMPS


def build(case):
    """(q, k, v, dO) of a case, bf16 on the CPU."""
    if case.kind == "ramp":
        return ramp_inputs(case.shape[1], case.scale, case.seed)
    return random_inputs(*case.shape, seed=case.seed, scale=case.scale)


def round_up_1sig(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


# 3 x the emulation's worst value over the group's cases, rounded up to one
# significant digit (test_attention_ref_cpu.py::test_tolerances_are_three_times_emulation)
TOL = {
    "grouped": dict(o=1e-02, o_q90=8e-03, dq=1e+00, dq_q90=9e-03, dk=3e-02, dk_q90=9e-03,
                    dv=2e-02, dv_q90=9e-03, lse2=3e-06, delta=2e-01),
    "reference": dict(o=1e-02, o_q90=8e-03, dq=4e-01, dq_q90=9e-03, dk=2e-02, dk_q90=9e-03,
                      dv=2e-02, dv_q90=9e-03, lse2=3e-06, delta=2e-01),
    "peaky": dict(o=8e-03, o_q90=6e-03, lse2=8e-05),
    "sm_scale": dict(o=1e-02, o_q90=8e-03, dq=3e-01, dq_q90=9e-03, dk=2e-02, dk_q90=9e-03,
                     dv=2e-02, dv_q90=9e-03, lse2=3e-06, delta=2e-01),
    "ramp": dict(o=9e-03, o_q90=8e-03, dq=6e-01, dq_q90=2e-01, dk=6e-02, dk_q90=2e-02,
                 dv=2e-02, dv_q90=9e-03, lse2=2e-05, delta=8e-02),
}


def bounded(case):
    """The keys of TOL that a case is held to."""
    return [n for n in TOL[case.group] if case.backward or n.split("_")[0] in FWD_QUANTITIES]


def check(case, got, ref):
    """Assert every bound of the case's group on `got` vs `ref`; prints each
    figure before it asserts.  Returns the figures."""
    e = errors(got, ref)
    tol = TOL[case.group]
    for n in bounded(case):
        print(f"{case.group} {case.id} {n}: {e[n]:.3e} (bound {tol[n]:.0e})")
    bad = [f"{n} {e[n]:.3e} > {tol[n]:.0e}" for n in bounded(case) if not e[n] <= tol[n]]
    assert not bad, f"{case.group} {case.id}: " + "; ".join(bad)
    return e

# derived, not measured (uniform scores: every p is exactly 1, l exactly s + 1)
UNIFORM_O_REL, UNIFORM_O_ABS = 2.0 ** -7, 1e-6   # one bf16 ulp
UNIFORM_LSE2_ABS = 1e-5
