"""Inputs, references, metric and wrong variants shared by the tests of the
fused elementwise / normalisation / loss / optimizer kernels of
src/ops/llama_ops.hip: the CPU test of the references themselves
(tests/test_ops_ref_cpu.py) and the GPU tests (tests/test_ops_gpu.py) build the
same cases here, on the CPU generator, so both see the same data.

ref64_*     the op in float64 on the (bf16) inputs, forward and backward, with
            `cond` next to every output (below).  Device-agnostic.
emulated_*  the same math in fp32 PyTorch, rounded to bf16 where a kernel
            stores bf16 (h of add_rms_norm before it is normalised; p / m / v
            of AdamW) and to fp32 where it stores fp32 (rstd, lse).  It sizes
            the tolerances and carries the MUTANTS; it is no copy of a kernel.

The metric, `check(got_bf16, ref64, cond64, c)`, is per element and derived:

    |got - ref| <= ulp_bf16(ref) + c * 2^-24 * cond

  * ulp_bf16(r) = 2^(floor(log2 |r|) - 7), the spacing of bf16 at r (for r = 0
    the ulp of the smallest non-zero magnitude of the tensor; never finer than
    bf16's smallest normal allows, 2^-133).  A correctly rounded result of an
    exact value is within half of it; the whole ulp covers a value that the
    fp32 error moved across a binade.
  * cond is the fp64 sum of the absolute values of the terms of the output's
    last sum or difference, which is where fp32 cancellation costs relative
    accuracy: |b1 m| + |(1-b1) g| for exp_avg, |p decay| + |step m / denom| for
    p, |r g| + |x coef| (+ |dres|) for dx, |x| + |delta| for h,
    sum_rows |dy x r| for dw, |softmax| + onehot (times the scale) for
    dlogits, |x1 cos| + |x2 sin| for RoPE, |dh u s| (1 + |g (1 - s)|) for
    dgate, |result| where nothing cancels (y, swiglu h and dup, exp_avg_sq).
  * c, the number of fp32 roundings (2^-24 relative each) granted on top:
      C_ELEM = 32 for elementwise outputs.  The longest chain is dgate:
        4 products, 2 sums, the reciprocal and v_exp_f32 (1 ulp each, the
        argument scaling of exp adds |g| log2(e) <= 12 roundings at |g| <= 8):
        about 20; rstd (v_rsq_f32, 1 ulp, on a sum of squares whose fp32 error
        grows like the square root of its length) and the AdamW division and
        square root need fewer.
      c = n for a sum of n fp32 terms (dw: n = N rows): the textbook
        (n - 1) * 2^-24 * sum |terms| for any order of summation, plus one
        rounding for the product inside each term.
  * the share of elements not bit-equal to the round-to-nearest bf16 of ref is
    at most SHARE_MAX = 2e-3, counted over the elements whose cond term is
    below a quarter of the ulp.  A mismatch needs the exact value within the
    fp32 error (at most 2^-19 relative) of a rounding boundary; boundaries are
    2^-8 relative apart, which gives about 2^-10.
  * the emulation itself stays within every bound on every case and at or
    below EMU_SHARE_MAX = 2e-4 per output over the op's cases
    (tests/test_ops_ref_cpu.py asserts it).

fp32 outputs (rstd, lse, per-row loss, mean loss) get 3 x the emulation's worst
error over all cases, rounded up to one significant digit: FP32_TOL.  None of
these numbers came from a kernel's output; tests/test_ops_ref_cpu.py measures
them again, prints them (pytest -s) and holds FP32_TOL to them.

Emulation vs fp64, as measured on the CPU: the worst element of any case as a
fraction of its bound, and the share not bit-equal over the op's cases pooled
(a dw has a few thousand elements, so one mismatch is already 2e-4 of a case):

   op, output                   worst error / bound  share not bit-equal
   rms_norm y                   0.500                6.7e-06
   rms_norm dx                  0.594                8.8e-06
   rms_norm dw                  0.500                5.6e-05
   add_rms_norm h               0.500                0.0e+00
   add_rms_norm y               0.500                6.3e-06
   add_rms_norm dx              0.500                1.6e-05
   add_rms_norm dw              0.500                5.6e-05
   swiglu h                     0.500                6.4e-06
   swiglu dgu                   0.500                8.2e-06
   rope_qkv qkv_out             0.500                8.0e-06
   rope_qkv dqkv                0.500                6.4e-06
   cross_entropy dlogits        0.500                2.8e-05
   adamw p                      0.500                2.5e-06
   adamw exp_avg                0.500                0.0e+00
   adamw exp_avg_sq             0.500                0.0e+00
   fp32 output                  worst error          bound (3 x, one digit, rounded up)
   rstd      (relative)         1.72e-07             6e-07
   lse       (/ max(1, |lse|))  6.59e-08             2e-07
   loss_rows (/ max(1, |lse|))  1.37e-07             5e-07
   loss      (absolute)         1.77e-06             6e-06

What the references define where the plain formula leaves a choice:
  * add_rms_norm: y and the backward are those of the STORED h, the bf16
    rounding of x + delta, since that is what the next layer reads.
  * cross_entropy: a row whose target is ignore_index OR lies outside [0, V)
    is ignored: loss 0, gradient 0, and it does not count in n_valid (the mean
    divides by the rows that contributed).  With every row ignored the loss is 0.
  * rope_qkv takes the fp32 cos / sin tables as inputs: the contract is the
    rotation, not the table.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
C_ELEM = 32
SHARE_MAX = 2e-3
EMU_SHARE_MAX = 2e-4
EPS = 1e-5


# --------------------------------------------------------------------- metric
def rne_bf16(r64):
    """Round-to-nearest-even bf16 of an fp64 tensor."""
    return r64.float().bfloat16()


def ulp_bf16(r64):
    a = r64.abs()
    nz = a[a > 0]
    floor = nz.min() if nz.numel() else a.new_tensor(2.0 ** -126)
    a = torch.where(a == 0, floor, a)
    e = torch.frexp(a)[1] - 1                       # floor(log2 a), exactly
    return torch.exp2((e.clamp_min(-126) - 7).double())


def figures(got, ref, cond, c=C_ELEM):
    """(worst |got - ref| / bound, share of counted elements not bit-equal to
    the rounded reference, number of counted elements)."""
    g = got.double()
    ulp = ulp_bf16(ref)
    slack = c * U32 * cond
    ratio = ((g - ref).abs() / (ulp + slack)).max().item() if g.numel() else 0.0
    counted = slack < 0.25 * ulp
    n = int(counted.sum().item())
    bad = int(((got != rne_bf16(ref)) & counted).sum().item())
    return ratio, (bad / n if n else 0.0), n


def check(got, ref, cond, c=C_ELEM, what="", share_max=SHARE_MAX):
    """Assert the metric of the module docstring on a bf16 tensor `got`;
    prints each figure before it asserts.  Returns (ratio, share, counted)."""
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape == cond.shape, what
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    assert torch.isfinite(ref).all(), f"{what}: non-finite reference"
    ratio, share, n = figures(got, ref, cond, c)
    print(f"{what}: worst error {ratio:.3f} of its bound, {share:.2e} of {n} not bit-equal (c = {c})")
    assert ratio <= 1.0, f"{what}: an element is {ratio:.3g} x its bound"
    assert share <= share_max, f"{what}: {share:.3e} of {n} elements not bit-equal (> {share_max:.0e})"
    return ratio, share, n


def round_up_1sig(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


# 3 x the emulation's worst value over all cases, rounded up to one significant
# digit (test_ops_ref_cpu.py::test_emulation_table).  rstd: relative.  lse and
# loss_rows (= lse - logit[target]): relative to max(1, |lse|), since fp32
# holds an lse of 300 no finer than 3e-5.  loss: absolute.
FP32_TOL = dict(rstd=6e-7, lse=2e-7, loss_rows=5e-7, loss=6e-6)


def fp32_error(name, got, ref):
    """The error of the fp32 output `name` as FP32_TOL bounds it; `ref` is the
    dict of the references."""
    d = (got.double() - ref[name]).abs()
    if name == "rstd":
        d = d / ref[name].abs()
    if name in ("lse", "loss_rows"):
        d = d / ref["lse"].abs().clamp_min(1.0)
    return d.max().item() if d.numel() else 0.0


def check_fp32(name, got, ref, what=""):
    assert got.dtype == torch.float32 and torch.isfinite(got).all(), f"{what} {name}"
    e = fp32_error(name, got, ref)
    print(f"{what} {name}: {e:.3e} (bound {FP32_TOL[name]:.0e})")
    assert e <= FP32_TOL[name], f"{what} {name}: {e:.3e} > {FP32_TOL[name]:.0e}"
    return e


def check_all(got, ref, cond, what, n_rows=None, share_max=SHARE_MAX, fp32=True):
    """`check` on every bf16 output that `got` holds (c = n_rows for dw, the sum
    over the rows, C_ELEM otherwise) and, with `fp32`, check_fp32 on every fp32
    one.  Returns {name: (ratio, share, counted)}."""
    res = {}
    for name in cond:
        if name in got:
            c = n_rows if name == "dw" else C_ELEM
            res[name] = check(got[name], ref[name], cond[name], c, f"{what} {name}", share_max)
    if fp32:
        for name in FP32_TOL:
            if name in got:
                check_fp32(name, got[name], ref, what)
    return res


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# -------------------------------------------------------------------- RMSNorm
def ref64_rms_norm(x, w, eps, dy=None, delta=None, dh=None):
    """rms_norm (delta None) or add_rms_norm in fp64.  Returns (ref, cond):
    y, rstd [, h] and, given dy, dx, dw.  add_rms_norm: dx is also ddelta and
    `dh`, the gradient of the h output, joins it."""
    xd, wd = x.double(), w.double()
    ref, cond = {}, {}
    if delta is not None:
        h = xd + delta.double()
        ref["h"], cond["h"] = h, xd.abs() + delta.double().abs()
        xd = rne_bf16(h).double()                    # the stored h
    r = (xd.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    ref["y"] = xd * r * wd
    cond["y"] = ref["y"].abs()
    ref["rstd"] = r.squeeze(-1)
    if dy is None:
        return ref, cond
    g = dy.double() * wd
    coef = (g * xd).mean(-1, keepdim=True) * r ** 3
    a, b = r * g, xd * coef
    ref["dx"], cond["dx"] = a - b, a.abs() + b.abs()
    if dh is not None:
        ref["dx"] = ref["dx"] + dh.double()
        cond["dx"] = cond["dx"] + dh.double().abs()
    t = dy.double() * xd * r
    ref["dw"], cond["dw"] = t.sum(0), t.abs().sum(0)
    return ref, cond


RMS_LANE_SLICE = 5   # the lane whose elements the "lane slice" mutant forgets


def emulated_rms_norm(x, w, eps, dy=None, delta=None, dh=None, mut=None):
    xf, wf = x.float(), w.float()
    out = {}
    if delta is not None:
        out["h"] = (xf + delta.float()).bfloat16()
        xf = out["h"].float()
    sq = xf * xf
    if mut == "lane_slice":   # one lane's 8-vectors (every 64th) missing from the sum
        D = x.shape[-1]
        keep = (torch.arange(D, device=x.device) // 8) % 64 != RMS_LANE_SLICE
        sq = sq * keep
    ms = sq.sum(-1, keepdim=True) / x.shape[-1]
    r = torch.rsqrt(ms + (0.0 if mut == "no_eps" else eps))
    out["y"] = (xf * r * wf).bfloat16()
    out["rstd"] = r.squeeze(-1)
    if dy is None:
        return out
    dyf = dy.float()
    g = dyf * wf
    coef = (g * xf).sum(-1, keepdim=True) * r * r * r / x.shape[-1]
    dx = r * g - (0.0 if mut == "dx_no_projection" else xf * coef)
    if dh is not None:
        dx = dx + dh.float()
    out["dx"] = dx.bfloat16()
    t = dyf * xf * (1.0 if mut == "dw_no_rstd" else r)
    dw = t.sum(0)
    if mut == "dw_last_row_dropped":
        dw = dw - t[-1]
    if mut == "dw_last_row_twice":
        dw = dw + t[-1]
    out["dw"] = dw.bfloat16()
    return out


RmsCase = namedtuple("RmsCase", "id N D kind backward seed")
# kinds: normal  x ~ N(0, 1)
#        small   x ~ 1e-3 N(0, 1): eps carries rstd
#        zero    normal with row 1 (of h, for add_rms_norm) all zero
#        spike   N = D / 8 rows, row i zero except its aligned 8-vector i: every
#                (lane, k) slot of every VPL / CPT layout carries a row's whole
#                energy once


def rms_case(N, D, kind="normal", backward=True):
    return RmsCase(f"{kind}_{N}x{D}" + ("" if backward else "_fwd"), N, D, kind, backward, 100 + N + D)


RMS_CASES = [
    # rmsnorm_bwd_kernel (grid cap 512 x 2 rows): N 1027 = a second iteration
    # on the other LDS parity buffer for workgroups 0 and 1, workgroup 1's
    # second iteration holding a dead tail row (row 1027)
    rms_case(1027, 2048), rms_case(1027, 4096), rms_case(1027, 8192),
    # colsum_stage1 with 17 partial rows (groups of 2, the last of 1, the rest
    # empty) and with 2 (groups of 1); N odd: a dead tail row in iteration 0
    rms_case(33, 4096), rms_case(3, 4096),
    # generic kernels: rmsnorm_bwd_generic_kernel's loop past 512 x 4 rows
    rms_case(2051, 136), rms_case(77, 136),
    # generic, 4 x 6144 x 4 B = 96 KiB of LDS: the hipFuncSetAttribute branch
    rms_case(2051, 6144),
    # rmsnorm_fwd_kernel's row loop past 4096 x 4 rows, generic and VPL
    rms_case(16389, 136, backward=False), rms_case(16389, 2048, backward=False),
    rms_case(33, 4096, "small"), rms_case(77, 136, "small"),
    rms_case(33, 4096, "zero"), rms_case(77, 136, "zero"),
    rms_case(256, 2048, "spike"), rms_case(512, 4096, "spike"), rms_case(1024, 8192, "spike"), rms_case(17, 136, "spike"),
]


def build_rms(case, add):
    """dict x, w, dy [, delta, dh] in bf16 on the CPU.  For add_rms_norm the
    kind describes h = x + delta."""
    N, D = case.N, case.D
    g = _gen(case.seed + (7 if add else 0))
    scale = 1e-3 if case.kind == "small" else 1.0
    x = scale * torch.randn(N, D, generator=g)
    if case.kind == "spike":
        assert N == D // 8
        keep = torch.zeros(N, D // 8, dtype=torch.bool)
        keep[torch.arange(N), torch.arange(N)] = True
        x = x * keep.repeat_interleave(8, dim=1)
    if case.kind == "zero":
        x[1] = 0.0
    t = dict(w=(1 + 0.1 * torch.randn(D, generator=g)).bfloat16())
    if add:
        delta = (scale * torch.randn(N, D, generator=g)).bfloat16()
        if case.kind in ("spike", "zero"):
            # h must have the pattern: x = pattern - delta, exactly, where h is zero
            hz = x.bfloat16().float()
            xx = (hz - delta.float()).bfloat16()
            zero = hz == 0
            xx = torch.where(zero, (-delta.float()).bfloat16(), xx)
            t.update(x=xx, delta=delta)
        else:
            t.update(x=x.bfloat16(), delta=delta)
        t["dh"] = torch.randn(N, D, generator=g).bfloat16()
    else:
        t["x"] = x.bfloat16()
    t["dy"] = torch.randn(N, D, generator=g).bfloat16()
    return t


def rms_conditions(case, t, ref):
    """The input conditions of a case, asserted on the reference."""
    h = rne_bf16(ref["h"]).double() if "h" in ref else t["x"].double()
    ms = h.pow(2).mean(-1)
    if case.kind == "small":
        assert (EPS / (ms + EPS)).min().item() > 0.5, "eps does not carry rstd"
    if case.kind == "zero":
        assert (h[1] == 0).all() and ms[0] > 0
    if case.kind == "spike":
        nz = (h != 0).view(case.N, case.D // 8, 8).any(-1)
        assert torch.equal(nz, torch.eye(case.N, dtype=torch.bool, device=nz.device)), "spike pattern"


# --------------------------------------------------------------------- SwiGLU
def ref64_swiglu(gu, dh=None):
    g, u = gu.double().chunk(2, -1)
    s = torch.sigmoid(g)
    ref = dict(h=g * s * u)
    cond = dict(h=ref["h"].abs())
    if dh is None:
        return ref, cond
    d = dh.double()
    k = g * (1 - s)
    dg, du = d * u * s * (1 + k), d * g * s
    ref["dgu"] = torch.cat([dg, du], -1)
    cond["dgu"] = torch.cat([(d * u * s).abs() * (1 + k.abs()), du.abs()], -1)
    return ref, cond


def emulated_swiglu(gu, dh=None, mut=None):
    g, u = gu.float().chunk(2, -1)
    s = torch.sigmoid(1.702 * g if mut == "sigmoid_1702" else g)
    out = dict(h=(g * s * u).bfloat16())
    if dh is None:
        return out
    d = dh.float()
    f = 1.0 if mut == "dgate_no_factor" else 1 + g * (1 - s)
    out["dgu"] = torch.cat([d * u * s * f, d * g * s], -1).bfloat16()
    return out


SwigluCase = namedtuple("SwigluCase", "id N F kind seed")
SWIGLU_CASES = [
    # 1032 * 16392 / 8 = 2,114,568 items > 8192 x 256: the grid-stride loop of
    # swiglu_fwd_kernel / swiglu_bwd_kernel runs a second trip; F % 64 != 0
    SwigluCase("loop_1032x16392", 1032, 16392, "normal", 41),
    SwigluCase("100x24", 100, 24, "normal", 42),
    # |g| up to 100, u and dh up to 2^60: no NaN, no inf
    SwigluCase("extreme_64x128", 64, 128, "extreme", 43),
]


def build_swiglu(case):
    g = _gen(case.seed)
    N, Fd = case.N, case.F
    if case.kind == "normal":
        return dict(gu=(2 * torch.randn(N, 2 * Fd, generator=g)).bfloat16(),
                    dh=torch.randn(N, Fd, generator=g).bfloat16())
    # extreme: gate on a grid over [-100, 100] (both ends present); u and dh
    # are +-2^k, k uniform in [0, 60] (k = 60 present).  fp32 math cannot hold
    # sigmoid(g) below g ~ -87.3 (it leaves fp32's normal range; from -88.7 on
    # e^-g overflows and 1 / (1 + e^-g) is 0), although silu(g) itself stays
    # a normal number down to g ~ -92.  The contract is fp32 math, so where
    # g < -86 u and dh are +-2^-20: every result is then below half of bf16's
    # smallest subnormal and 0 is its correct rounding; what the case holds
    # there is that the kernel returns that 0 and no NaN.
    gate = torch.linspace(-100, 100, N * Fd).view(N, Fd)[:, torch.randperm(Fd, generator=g)]
    def pow2():
        k = torch.randint(0, 61, (N, Fd), generator=g)
        k.view(-1)[::97] = 60
        sign = torch.randint(0, 2, (N, Fd), generator=g) * 2 - 1
        return torch.where(gate < -86, sign * 2.0 ** -20, sign * torch.exp2(k.double()))
    gu = torch.cat([gate.double(), pow2()], -1).bfloat16()
    return dict(gu=gu, dh=pow2().bfloat16())


def swiglu_conditions(case, t):
    if case.kind == "extreme":
        g, u = t["gu"].float().chunk(2, -1)
        assert g.min() == -100 and g.max() == 100
        assert u.abs().max() == 2.0 ** 60 and t["dh"].float().abs().max() == 2.0 ** 60


# ----------------------------------------------------------------------- RoPE
def _rot(x, c, s, sign):
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    val = torch.cat([x1 * c - sign * x2 * s, x2 * c + sign * x1 * s], -1)
    cnd = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return val, cnd


def _rope(qkv, cos, sin, H, KV, sign, shift=0):
    """Rotation of the q and k heads of [B, S, (H + 2 KV) * hd] by sign * angle
    (v untouched), packed like the input."""
    B, S, W = qkv.shape
    hd = W // (H + 2 * KV)
    x = qkv.view(B, S, H + 2 * KV, hd)
    c = cos.to(qkv.dtype).roll(shift, 0)[None, :, None, :]
    s = sin.to(qkv.dtype).roll(shift, 0)[None, :, None, :]
    val, cnd = _rot(x[:, :, :H + KV], c, s, sign)
    v = x[:, :, H + KV:]
    return torch.cat([val, v], 2).view(B, S, W), torch.cat([cnd, v.abs()], 2).view(B, S, W)


def split_qkv(packed, H, KV):
    B, S, W = packed.shape
    hd = W // (H + 2 * KV)
    q, k, v = packed.split([H * hd, KV * hd, KV * hd], -1)
    return q.reshape(B, S, H, hd), k.reshape(B, S, KV, hd), v.reshape(B, S, KV, hd)


def ref64_rope_qkv(qkv, cos, sin, H, KV, dqkv_out=None):
    """ref / cond of `qkv_out` (rotated q | k and v, packed [B, S, W]; split
    with split_qkv) and, given the packed output gradient, of `dqkv`."""
    ref, cond = {}, {}
    ref["qkv_out"], cond["qkv_out"] = _rope(qkv.double(), cos, sin, H, KV, 1.0)
    if dqkv_out is not None:
        ref["dqkv"], cond["dqkv"] = _rope(dqkv_out.double(), cos, sin, H, KV, -1.0)
    return ref, cond


def emulated_rope_qkv(qkv, cos, sin, H, KV, dqkv_out=None, mut=None):
    shift = 1 if mut == "position_off_by_one" else 0
    out = dict(qkv_out=_rope(qkv.float(), cos, sin, H, KV, 1.0, shift)[0].bfloat16())
    if dqkv_out is not None:
        sign = 1.0 if mut == "bwd_forward_sign" else -1.0
        out["dqkv"] = _rope(dqkv_out.float(), cos, sin, H, KV, sign, shift)[0].bfloat16()
    return out


RopeCase = namedtuple("RopeCase", "id B S H KV hd seed")
ROPE_CASES = [
    # 3 * 10924 * 8 * 8 = 2,097,408 items > 8192 x 256: rope_kernel's
    # grid-stride loop runs a second trip, on tokens of batch 2 (t % S wraps)
    RopeCase("loop_3x10924x4x2x128", 3, 10924, 4, 2, 128, 51),
    RopeCase("1x37x4x2x32", 1, 37, 4, 2, 32, 52),
    RopeCase("ch1_2x64x2x1x16", 2, 64, 2, 1, 16, 53),   # CH = 1: one chunk per half
]


def rope_tables(S, hd, theta=500000.0):
    """fp32 tables [S, hd / 2], the formula of dynolog_amd.models.llama."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    f = torch.outer(torch.arange(S, dtype=torch.float32), inv)
    return f.cos(), f.sin()


def build_rope(case):
    g = _gen(case.seed)
    W = (case.H + 2 * case.KV) * case.hd
    cos, sin = rope_tables(case.S, case.hd)
    return dict(qkv=torch.randn(case.B, case.S, W, generator=g).bfloat16(), cos=cos, sin=sin,
                dqkv_out=torch.randn(case.B, case.S, W, generator=g).bfloat16())


# -------------------------------------------------------------- cross-entropy
def xent_valid(tgt, V, ignore_index):
    return (tgt != ignore_index) & (tgt >= 0) & (tgt < V)


def ref64_cross_entropy(logits, tgt, ignore_index=-100, grad_loss=1.0):
    """Mean NLL over the valid rows (module docstring).  ref: loss, loss_rows,
    lse, n_valid, dlogits (the gradient of grad_loss * loss); cond: dlogits."""
    x = logits.double()
    N, V = x.shape
    valid = xent_valid(tgt, V, ignore_index)
    lse = torch.logsumexp(x, -1)
    safe = torch.where(valid, tgt, torch.zeros_like(tgt))
    rows = torch.where(valid, lse - x.gather(1, safe[:, None]).squeeze(1), torch.zeros_like(lse))
    n_valid = valid.sum().double()
    scale = valid.double()[:, None] * grad_loss / n_valid.clamp_min(1.0)
    p = torch.exp(x - lse[:, None])
    hot = F.one_hot(safe, V).double()
    ref = dict(loss=rows.sum() / n_valid.clamp_min(1.0), loss_rows=rows, lse=lse, n_valid=n_valid,
               dlogits=(p - hot) * scale)
    return ref, dict(dlogits=(p + hot) * scale)


def emulated_cross_entropy(logits, tgt, ignore_index=-100, grad_loss=1.0, mut=None):
    x = logits.float()
    N, V = x.shape
    valid = xent_valid(tgt, V, ignore_index)
    lse = torch.logsumexp(x, -1)                     # stored in fp32, read by the backward
    safe = torch.where(valid, tgt, torch.zeros_like(tgt))
    rows = torch.where(valid, lse - x.gather(1, safe[:, None]).squeeze(1), torch.zeros_like(lse))
    n_valid = valid.sum().float().clamp_min(1.0)
    div = float(N) if mut == "scale_1_over_N" else n_valid
    gl = 1.0 if mut == "grad_loss_ignored" else grad_loss
    scale = valid.float()[:, None] * (gl / div)
    hot = F.one_hot((safe + 1) % V if mut == "onehot_one_column_off" else safe, V).float()
    return dict(loss=rows.sum() / n_valid, loss_rows=rows, lse=lse,
                dlogits=((torch.exp(x - lse[:, None]) - hot) * scale).bfloat16())


XentCase = namedtuple("XentCase", "id N V kind ignore_index grad_loss seed")
# kinds: plain    logits ~ 3 N(0, 1); every 7th row's target is ignore_index, rows
#                 0 and 2 have the targets 0 and V - 1
#        all_ign  every target is ignore_index: loss 0, dlogits 0, no NaN
#        shift    odd rows shifted by +300: every lane's first vector sets a
#                 running max of ~300 that the combine steps carry
#        masked   columns 1920..2047 are -inf (a vocabulary padded to a multiple
#                 of 128 and masked): lanes 240..255 see nothing but -inf
#        oob      plain, and rows 4, 9 have the out-of-range target -1, row 5 the
#                 target V, none of them ignore_index: ignored AND not counted


def xent_case(N, V, kind="plain", ignore_index=-100, grad_loss=1.0, tag=""):
    return XentCase(f"{tag}{kind}_{N}x{V}", N, V, kind, ignore_index, grad_loss, 600 + N + V + len(kind))


XENT_CASES = [
    xent_case(37, 8),                                   # one vector per row: 255 idle lanes stay at (-inf, 0)
    xent_case(300, 512),
    xent_case(33, 2056, grad_loss=0.37),                # 257 vectors: lane 0 takes a second one; grad_loss != 1
    xent_case(64, 128256, grad_loss=0.37),              # the production vocabulary
    xent_case(300, 512, ignore_index=3, grad_loss=0.37, tag="ign3_"),   # ignore_index is a real class
    xent_case(16, 512, "all_ign"),
    xent_case(40, 512, "shift"),
    xent_case(24, 2048, "masked"),
    xent_case(40, 512, "oob", grad_loss=0.37),
    # N, V multiples of 128: through ops.linear the tiled xent_bwd_t_kernel runs
    xent_case(128, 256, tag="tiled_", grad_loss=0.37),
]


def build_xent(case):
    g = _gen(case.seed)
    N, V = case.N, case.V
    logits = 3 * torch.randn(N, V, generator=g)
    tgt = torch.randint(0, V, (N,), generator=g)
    if case.ignore_index >= 0:   # a real class: make sure some rows have it, by chance or not
        tgt[1::5] = case.ignore_index
    tgt[::7] = case.ignore_index
    tgt[1], tgt[2] = 0, V - 1
    if case.kind == "all_ign":
        tgt[:] = case.ignore_index
    if case.kind == "shift":
        logits[1::2] += 300
    if case.kind == "masked":
        logits[:, 1920:] = float("-inf")
        tgt = tgt.clamp_max(1919)
        tgt[::7] = case.ignore_index
    if case.kind == "oob":
        tgt[4] = tgt[9] = -1
        tgt[5] = V
    return dict(logits=logits.bfloat16(), tgt=tgt)


def xent_conditions(case, t, ref):
    N, V = case.N, case.V
    valid = xent_valid(t["tgt"], V, case.ignore_index)
    if case.kind == "all_ign":
        assert not valid.any() and ref["loss"] == 0 and (ref["dlogits"] == 0).all()
        return
    assert valid.any() and not valid.all()
    assert (t["tgt"][valid] == 0).any()
    assert (t["tgt"][valid] == V - 1).any() or case.kind == "masked"
    if case.kind == "oob":
        assert ref["n_valid"] < (t["tgt"] != case.ignore_index).sum()
    if case.kind == "masked":
        assert torch.isfinite(ref["loss"]) and torch.isinf(t["logits"].float()[:, 1920:]).all()
    if case.kind == "shift":
        assert ref["lse"].max() > 300


# ---------------------------------------------------------------------- AdamW
def ref64_adamw_step(p, g, m, v, step, lr, betas, eps, wd):
    """One AdamW step in fp64 on the (bf16) state: adamw_reference_step of
    dynolog_amd.ops.optim on float64 tensors, plus cond.  ref / cond: p,
    exp_avg, exp_avg_sq."""
    from dynolog_amd.ops.optim import adamw_reference_step
    pd, gd, md, vd = (t.double() for t in (p, g, m, v))
    p2, m2, v2 = adamw_reference_step(pd, gd, md, vd, step, lr, betas, eps, wd)
    b1, b2 = betas
    upd = lr / (1 - b1 ** step) * m2 / (v2.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    ref = dict(p=p2, exp_avg=m2, exp_avg_sq=v2)
    cond = dict(p=(pd * (1 - lr * wd)).abs() + upd.abs(),
                exp_avg=(b1 * md).abs() + ((1 - b1) * gd).abs(), exp_avg_sq=v2.abs())
    return ref, cond


def emulated_adamw_step(p, g, m, v, step, lr, betas, eps, wd, mut=None):
    b1, b2 = betas
    pf, gf, mf, vf = (t.float() for t in (p, g, m, v))
    if mut == "step_off_by_one":
        step = step - 1
    bc1 = 1.0 if mut == "no_bias_correction1" else 1 - b1 ** step
    bc2 = 1.0 if mut == "no_bias_correction2" else 1 - b2 ** step
    m2 = b1 * mf + (1 - b1) * gf
    v2 = b2 * vf + (1 - b2) * gf * gf
    denom = v2.sqrt() / math.sqrt(bc2) + eps
    p2 = pf * (1.0 if mut == "no_weight_decay" else 1 - lr * wd) - lr / bc1 * m2 / denom
    return dict(p=p.clone() if mut == "p_not_written" else p2.bfloat16(), exp_avg=m2.bfloat16(),
                exp_avg_sq=((4 * v2) if mut == "v_times_4" else v2).bfloat16())


def _f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


# The launcher takes the hyper-parameters as C floats, so the cases use the
# fp32 neighbours of the usual decimal values: the reference and the kernel
# then start from the same numbers.  The betas are near the usual 0.9 / 0.95
# but no short decimals: (9 m + g) / 10 of two bf16 values is an exact tie
# between two bf16 neighbours for 0.5 % of the elements (19 v + g^2 over 20 for
# 0.02 %), and which way a tie falls is decided by how 0.9 is represented, not
# by the update, so the bit-equal share would measure the representation.  The
# emulation showed this (0.5 % at 0.9, none at 0.9003); the update itself is
# the same code for any beta.
AdamCase = namedtuple("AdamCase", "id lr wd eps gscale seed")
ADAM_BETAS = (_f32(0.9003), _f32(0.9497))
ADAM_STEP0 = 7        # the state is that of a run 7 steps old
ADAM_CASES = [
    AdamCase("main", _f32(1e-3), _f32(0.1), _f32(1e-8), 1.0, 71),   # p ~ 0.02 N(0, 1): the step moves > 90 % of bf16 p
    AdamCase("wd0", _f32(1e-3), 0.0, _f32(1e-8), 1.0, 72),
    AdamCase("eps_carries", _f32(1e-3), _f32(0.1), _f32(1e-3), 1e-3, 73),   # g ~ 1e-3 N(0, 1): eps ~ sqrt(v)
]
ADAM_ZEROS = 16       # the first elements have g = m = v = 0: they only decay


def adam_state(case, n):
    """(p, m, v) flat bf16 of n elements, a mid-training state."""
    g = _gen(case.seed)
    p = (0.02 * torch.randn(n, generator=g)).bfloat16()
    m = (0.5 * case.gscale * torch.randn(n, generator=g)).bfloat16()
    v = (case.gscale ** 2 * (0.1 + torch.randn(n, generator=g).pow(2))).bfloat16()
    m[:ADAM_ZEROS] = 0
    v[:ADAM_ZEROS] = 0
    return p, m, v


def adam_grad(case, n, step):
    g = (case.gscale * torch.randn(n, generator=_gen(case.seed + 1000 * step))).bfloat16()
    g[:ADAM_ZEROS] = 0
    return g


def adam_hyper(case):
    return dict(lr=case.lr, betas=ADAM_BETAS, eps=case.eps, weight_decay=case.wd)


# -------------------------------------------------------------------- mutants
# op -> names of the wrong variants of its emulation (the `mut` argument).
# tests/test_ops_ref_cpu.py shows that `check` rejects each on at least one
# case of the op, i.e. that the GPU tests would fail for such a kernel.
MUTANTS = {
    "rms_norm": ["no_eps", "lane_slice", "dx_no_projection", "dw_no_rstd", "dw_last_row_dropped",
                 "dw_last_row_twice"],
    "swiglu": ["dgate_no_factor", "sigmoid_1702"],
    "rope_qkv": ["position_off_by_one", "bwd_forward_sign"],
    "cross_entropy": ["scale_1_over_N", "grad_loss_ignored", "onehot_one_column_off"],
    "adamw": ["p_not_written", "no_weight_decay", "no_bias_correction1", "no_bias_correction2",
              "v_times_4", "step_off_by_one"],
}
