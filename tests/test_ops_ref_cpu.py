"""The references, inputs and metric of the fused-op tests, checked on the CPU:
every ref64_* of tests/ops_cases.py against fp64 autograd of the plain PyTorch
expression, the emulation against the metric on every case (the table of the
module docstring, printed with `pytest -s`), the conditions the inputs have to
meet, and that `check` rejects every named wrong variant.  No kernel runs here;
tests/test_ops_gpu.py holds src/ops/llama_ops.hip to the same cases."""
import pytest
import torch
import torch.nn.functional as F

import ops_cases as C

MUTANT_MAX_ELEMS = 1 << 19   # the wrong variants are tried on the small cases only


def _leaf(t):
    return t.detach().double().requires_grad_(True)


# ------------------------------------------------- ref64 vs fp64 autograd
@pytest.mark.parametrize("add", [False, True], ids=["rms_norm", "add_rms_norm"])
@pytest.mark.parametrize("case", [C.RMS_CASES[6], C.RMS_CASES[11], C.RMS_CASES[13]], ids=lambda c: c.id)
def test_ref64_rms_norm_matches_autograd(case, add):
    t = C.build_rms(case, add)
    ref, _ = C.ref64_rms_norm(t["x"], t["w"], C.EPS, t["dy"], t.get("delta"), t.get("dh"))
    x, w = _leaf(t["x"]), _leaf(t["w"])
    leaves, outs, grads = [x, w], [], []
    h = x
    if add:
        d = _leaf(t["delta"])
        leaves.append(d)
        h = x + d
        outs.append(h)
        grads.append(t["dh"].double())
        assert (h - ref["h"]).abs().max().item() == 0
        h = h + (C.rne_bf16(h.detach()).double() - h.detach())   # the stored h, straight through
    y = F.rms_norm(h, (case.D,), w, C.EPS)
    g = torch.autograd.grad(outs + [y], leaves, grads + [t["dy"].double()])
    assert (y - ref["y"]).abs().max().item() < 1e-10
    assert (g[0] - ref["dx"]).abs().max().item() < 1e-10
    assert (g[1] - ref["dw"]).abs().max().item() < 1e-10
    if add:
        assert (g[2] - ref["dx"]).abs().max().item() < 1e-10
    ms = h.detach().pow(2).mean(-1)
    assert (ref["rstd"] * (ms + C.EPS).sqrt() - 1).abs().max().item() < 1e-12


@pytest.mark.parametrize("case", C.SWIGLU_CASES[1:], ids=lambda c: c.id)
def test_ref64_swiglu_matches_autograd(case):
    t = C.build_swiglu(case)
    ref, _ = C.ref64_swiglu(t["gu"], t["dh"])
    gu = _leaf(t["gu"])
    a, b = gu.chunk(2, -1)
    h = F.silu(a) * b
    (dgu,) = torch.autograd.grad(h, gu, t["dh"].double())
    for got, want in ((h, ref["h"]), (dgu, ref["dgu"])):
        rel = ((got - want).abs() / want.abs().clamp_min(1e-300)).max().item()
        assert rel < 1e-10, rel


@pytest.mark.parametrize("case", C.ROPE_CASES[1:], ids=lambda c: c.id)
def test_ref64_rope_matches_complex_rotation(case):
    """The rotate-half convention as a complex product (x1 + i x2)(cos + i sin),
    its backward by autograd; v and its gradient pass through untouched."""
    t = C.build_rope(case)
    H, KV, hd = case.H, case.KV, case.hd
    ref, _ = C.ref64_rope_qkv(t["qkv"], t["cos"], t["sin"], H, KV, t["dqkv_out"])
    qkv = _leaf(t["qkv"])
    x = qkv.view(case.B, case.S, H + 2 * KV, hd)
    z = torch.complex(x[..., :hd // 2], x[..., hd // 2:])
    rot = z * torch.complex(t["cos"].double(), t["sin"].double())[None, :, None, :]
    rot = torch.cat([rot.real, rot.imag], -1)
    out = torch.cat([rot[:, :, :H + KV], x[:, :, H + KV:]], 2).view(qkv.shape)
    (dqkv,) = torch.autograd.grad(out, qkv, t["dqkv_out"].double())
    assert (out - ref["qkv_out"]).abs().max().item() < 1e-10
    assert (dqkv - ref["dqkv"]).abs().max().item() < 1e-10
    vcols = slice((H + KV) * hd, None)
    assert torch.equal(ref["qkv_out"][..., vcols], t["qkv"].double()[..., vcols])
    assert torch.equal(ref["dqkv"][..., vcols], t["dqkv_out"].double()[..., vcols])


@pytest.mark.parametrize("case", [c for c in C.XENT_CASES if c.V <= 4096], ids=lambda c: c.id)
def test_ref64_cross_entropy_matches_torch(case):
    """F.cross_entropy in fp64, the out-of-range targets mapped to ignore_index
    (the meaning the module docstring gives them)."""
    t = C.build_xent(case)
    ref, _ = C.ref64_cross_entropy(t["logits"], t["tgt"], case.ignore_index, case.grad_loss)
    x = _leaf(t["logits"])
    valid = C.xent_valid(t["tgt"], case.V, case.ignore_index)
    tg = torch.where(valid, t["tgt"], torch.full_like(t["tgt"], case.ignore_index))
    rows = F.cross_entropy(x, tg, ignore_index=case.ignore_index, reduction="none")
    assert (rows - ref["loss_rows"]).abs().max().item() < 1e-10
    assert (torch.logsumexp(x, -1) - ref["lse"]).abs().max().item() < 1e-10
    if valid.any():
        loss = F.cross_entropy(x, tg, ignore_index=case.ignore_index)
        (dx,) = torch.autograd.grad(loss * case.grad_loss, x)
        assert abs(loss.item() - ref["loss"].item()) < 1e-10
        assert (dx - ref["dlogits"]).abs().max().item() < 1e-10
    else:   # torch's mean over no rows is NaN; ours is 0
        assert ref["loss"].item() == 0 and (ref["dlogits"] == 0).all()


@pytest.mark.parametrize("case", C.ADAM_CASES, ids=lambda c: c.id)
def test_ref64_adamw_matches_torch_optim(case):
    n = 4096
    p, m, v = C.adam_state(case, n)
    step = C.ADAM_STEP0 + 1
    g = C.adam_grad(case, n, step)
    hp = C.adam_hyper(case)
    ref, _ = C.ref64_adamw_step(p, g, m, v, step, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
    q = torch.nn.Parameter(p.double())
    opt = torch.optim.AdamW([q], **hp)
    opt.state[q] = dict(step=torch.tensor(float(C.ADAM_STEP0)), exp_avg=m.double(), exp_avg_sq=v.double())
    q.grad = g.double()
    opt.step()
    assert (q.detach() - ref["p"]).abs().max().item() < 1e-10
    assert (opt.state[q]["exp_avg"] - ref["exp_avg"]).abs().max().item() < 1e-10
    assert (opt.state[q]["exp_avg_sq"] - ref["exp_avg_sq"]).abs().max().item() < 1e-10
    # the fp32 form that dynolog_amd.ops.optim keeps is the same function
    from dynolog_amd.ops.optim import adamw_reference_step
    p32 = adamw_reference_step(p.float(), g.float(), m.float(), v.float(), step, hp["lr"], hp["betas"],
                               hp["eps"], hp["weight_decay"])[0]
    assert (p32.double() - ref["p"]).abs().max().item() < 1e-6


# ------------------------------------------------- the metric itself
def test_ulp_bf16_and_check():
    r = torch.tensor([1.0, 1.99, 2.0, -0.75, 0.0, 3e-39], dtype=torch.float64)
    u = C.ulp_bf16(r)
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133]
    ref = torch.tensor([1.0, 1.0 + 2.0 ** -9, 100.0], dtype=torch.float64)
    cond = ref.abs()
    C.check(C.rne_bf16(ref), ref, cond, what="exact")
    off = C.rne_bf16(ref).clone()
    off[2] = 101.0   # 2 ulp
    with pytest.raises(AssertionError):
        C.check(off, ref, cond, what="two ulp off")
    one = C.rne_bf16(ref).clone()
    one[0] = 1.0 + 2.0 ** -7   # within the bound, but not the rounded reference
    with pytest.raises(AssertionError):
        C.check(one, ref, cond, what="one ulp off, share")
    # cancellation: the cond term admits what the ulp of a tiny result does not
    C.check(torch.tensor([2.0 ** -20]).bfloat16(), torch.tensor([0.0], dtype=torch.float64),
            torch.tensor([64.0], dtype=torch.float64), what="cancelled")


# ------------------------------------------------- emulation on every case
def _eval(op, case, t, mut=None):
    """(got, n_rows) of the emulation of `op`."""
    if op in ("rms_norm", "add_rms_norm"):
        dy = t["dy"] if case.backward else None
        return C.emulated_rms_norm(t["x"], t["w"], C.EPS, dy, t.get("delta"),
                                   t.get("dh") if case.backward else None, mut=mut)
    if op == "swiglu":
        return C.emulated_swiglu(t["gu"], t["dh"], mut=mut)
    if op == "rope_qkv":
        return C.emulated_rope_qkv(t["qkv"], t["cos"], t["sin"], case.H, case.KV, t["dqkv_out"], mut=mut)
    if op == "cross_entropy":
        return C.emulated_cross_entropy(t["logits"], t["tgt"], case.ignore_index, case.grad_loss, mut=mut)
    hp = C.adam_hyper(case)
    return C.emulated_adamw_step(t["p"], t["g"], t["m"], t["v"], t["step"], hp["lr"], hp["betas"], hp["eps"],
                                 hp["weight_decay"], mut=mut)


def _reference(op, case):
    """(inputs, ref, cond, n_rows) of a case, its input conditions asserted."""
    if op in ("rms_norm", "add_rms_norm"):
        t = C.build_rms(case, op == "add_rms_norm")
        dy = t["dy"] if case.backward else None
        ref, cond = C.ref64_rms_norm(t["x"], t["w"], C.EPS, dy, t.get("delta"),
                                     t.get("dh") if case.backward else None)
        C.rms_conditions(case, t, ref)
        return t, ref, cond, case.N
    if op == "swiglu":
        t = C.build_swiglu(case)
        C.swiglu_conditions(case, t)
        return (t,) + C.ref64_swiglu(t["gu"], t["dh"]) + (None,)
    if op == "rope_qkv":
        t = C.build_rope(case)
        return (t,) + C.ref64_rope_qkv(t["qkv"], t["cos"], t["sin"], case.H, case.KV, t["dqkv_out"]) + (None,)
    if op == "cross_entropy":
        t = C.build_xent(case)
        ref, cond = C.ref64_cross_entropy(t["logits"], t["tgt"], case.ignore_index, case.grad_loss)
        C.xent_conditions(case, t, ref)
        return t, ref, cond, None
    n = 1 << 18
    p, m, v = C.adam_state(case, n)
    step = C.ADAM_STEP0 + 1
    t = dict(p=p, m=m, v=v, g=C.adam_grad(case, n, step), step=step)
    hp = C.adam_hyper(case)
    ref, cond = C.ref64_adamw_step(p, t["g"], m, v, step, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
    return t, ref, cond, None


OPS = [("rms_norm", C.RMS_CASES), ("add_rms_norm", C.RMS_CASES), ("swiglu", C.SWIGLU_CASES),
       ("rope_qkv", C.ROPE_CASES), ("cross_entropy", C.XENT_CASES), ("adamw", C.ADAM_CASES)]
ALL = [(op, c) for op, cases in OPS for c in cases]
_small = {}   # (op, case id) -> (inputs, ref, cond, n_rows), kept for the mutant tests


def _numel(t):
    return max(x.numel() for x in t.values() if torch.is_tensor(x))


@pytest.fixture(scope="module")
def table():
    """{(op, output): [worst bound ratio, worst share]} and {fp32 name: worst
    error} of the emulation, filled by test_emulation_within_metric."""
    return {}, {}


@pytest.mark.parametrize("op,case", ALL, ids=[f"{op}-{c.id}" for op, c in ALL])
def test_emulation_within_metric(op, case, table):
    t, ref, cond, n_rows = _reference(op, case)
    if _numel(t) <= MUTANT_MAX_ELEMS:
        _small[(op, case.id)] = (t, ref, cond, n_rows)
    got = _eval(op, case, t)
    # every bound per case; the share per case only at the kernels' SHARE_MAX:
    # a dw has a few thousand elements, where one mismatch is already 2e-4, so
    # EMU_SHARE_MAX is held on the op's cases pooled (test_emulation_table)
    res = C.check_all(got, ref, cond, f"{op} {case.id}", n_rows, fp32=False)
    bf, fp = table
    for name, (ratio, share, n) in res.items():
        w = bf.setdefault((op, name), [0.0, 0.0, 0])
        w[0], w[1], w[2] = max(w[0], ratio), w[1] + share * n, w[2] + n
    for name in C.FP32_TOL:
        if name in got:
            fp[name] = max(fp.get(name, 0.0), C.fp32_error(name, got[name], ref))


def test_adamw_main_case_moves_most_parameters():
    t, ref, _, _ = _reference("adamw", C.ADAM_CASES[0])
    moved = (C.rne_bf16(ref["p"]) != t["p"]).double().mean().item()
    print(f"the fp64 step changes the bf16 value of {100 * moved:.1f} % of p")
    assert moved > 0.9
    z = slice(0, C.ADAM_ZEROS)   # g = m = v = 0: decay only, finite
    hp = C.adam_hyper(C.ADAM_CASES[0])
    assert torch.equal(ref["p"][z], t["p"][z].double() * (1 - hp["lr"] * hp["weight_decay"]))
    case = C.ADAM_CASES[2]       # eps carries the denominator
    t, ref, _, _ = _reference("adamw", case)
    share = case.eps / (ref["exp_avg_sq"][C.ADAM_ZEROS:].sqrt() / (1 - C.ADAM_BETAS[1] ** 8) ** 0.5 + case.eps)
    assert share.median().item() > 0.3


def test_emulation_table(table):
    """Prints the table of the module docstring.  Holds the emulation's share
    of elements not bit-equal to EMU_SHARE_MAX, per output over the op's
    cases, and FP32_TOL to 3 x the emulation's worst error, rounded up to one
    significant digit (the worst value is given 10 % either way: fp32 sums may
    differ in the last bits from one BLAS to the next)."""
    bf, fp = table
    if not bf:
        pytest.skip("selected alone: the table is filled by test_emulation_within_metric")
    assert len(bf) == 15 and set(fp) == set(C.FP32_TOL), \
        "needs the whole of test_emulation_within_metric, passing, in the same run"
    print()
    print(f"   {'op, output':28s} {'worst error / bound':20s} share not bit-equal")
    for (op, name), (ratio, bad, n) in bf.items():
        print(f"   {op + ' ' + name:28s} {ratio:<20.3f} {bad / n:.1e}")
    for (op, name), (ratio, bad, n) in bf.items():
        assert bad / n <= C.EMU_SHARE_MAX, f"{op} {name}: {bad / n:.2e} of {n}"
    print(f"   {'fp32 output':28s} {'worst error':20s} bound")
    for name, x in fp.items():
        print(f"   {name:28s} {x:<20.2e} {C.FP32_TOL[name]:.0e}")
        lo, hi = C.round_up_1sig(3 * x * 0.9), C.round_up_1sig(3 * x * 1.1)
        assert lo * (1 - 1e-9) <= C.FP32_TOL[name] <= hi * (1 + 1e-9), \
            f"{name}: bound {C.FP32_TOL[name]:.0e}, 3 x emulation worst = {3 * x:.3e}"


# ------------------------------------------------- every mutant is rejected
MUT = [(op, m) for op, ms in C.MUTANTS.items() for m in ms]


@pytest.mark.parametrize("op,mut", MUT, ids=[f"{op}-{m}" for op, m in MUT])
def test_mutant_is_rejected(op, mut):
    """`check` fails the wrong variant on at least one (small) case of its op:
    a kernel wrong in this way would fail tests/test_ops_gpu.py."""
    cases = dict(OPS)[op]
    rejected = []
    for case in cases:
        key = (op, case.id)
        if key not in _small:
            probe = _reference(op, case)
            if _numel(probe[0]) > MUTANT_MAX_ELEMS:
                continue
            _small[key] = probe
        t, ref, cond, n_rows = _small[key]
        got = _eval(op, case, t, mut=mut)
        try:
            C.check_all(got, ref, cond, f"{op} {case.id} [{mut}]", n_rows)
        except AssertionError:
            rejected.append(case.id)
    print(f"{op} {mut}: rejected on {len(rejected)} cases: {rejected}")
    assert rejected, f"{op} {mut} passes every case"
