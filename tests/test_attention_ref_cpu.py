"""The references and inputs of the attention tests, checked on the CPU:
ref64 against PyTorch's own SDPA in fp64, the emulation errors that the GPU
tolerances are taken from (printed with `pytest -s`), and the conditions the
inputs have to meet for the per-row metric to mean something.  No kernel runs
here; tests/test_attention_gpu.py holds src/ops/attention.hip to these."""
import pytest
import torch
import torch.nn.functional as F

import attention_cases as A

KEYS = ("o", "o_q90", "dq", "dq_q90", "dk", "dk_q90", "dv", "dv_q90", "lse2", "delta")
FLOORED_CAP = 0.02


@pytest.fixture(scope="module")
def measured():
    """{case id: (case, inputs, fp64 reference, emulation errors)}, computed once."""
    out = {}
    for c in A.ALL_CASES:
        q, k, v, do = A.build(c)
        ref = A.ref64_all(q, k, v, do, c.sm_scale)
        emu = A.emulated(q, k, v, c.sm_scale, do)
        out[c.group + " " + c.id] = (c, (q, k, v, do), ref, A.errors(emu, ref))
    return out


def test_case_ids_are_unique():
    ids = [c.group + " " + c.id for c in A.ALL_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("B,S,H,KV,sm_scale", [(2, 128, 6, 2, A.DEFAULT_SCALE), (1, 256, 4, 4, 0.25)])
def test_ref64_matches_sdpa(B, S, H, KV, sm_scale):
    q, k, v, do = A.random_inputs(B, S, H, KV, seed=3)
    ref = A.ref64_all(q, k, v, do, sm_scale)
    qd, kd, vd = (t.double().transpose(1, 2).requires_grad_(True) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qd, kd, vd, is_causal=True, scale=sm_scale, enable_gqa=True)
    dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), do.double().transpose(1, 2))
    for name, a in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        err = (a.transpose(1, 2) - ref[name]).abs().max().item()
        assert err < 1e-10, f"{name}: {err:.3g}"
    # lse2: exp2(scaled base-2 scores - lse2) sums to 1 over the causal keys
    z2 = torch.einsum("bihd,bjhd->bhij", q.double(), k.double().repeat_interleave(H // KV, dim=2))
    z2 = z2 * sm_scale * A.LOG2E
    p = torch.exp2(z2 - ref["lse2"][..., None]).tril()
    assert (p.sum(-1) - 1).abs().max().item() < 1e-10
    # delta = rowsum(dO * O) = rowsum(P * dP)
    dp = torch.einsum("bihd,bjhd->bhij", do.double(), v.double().repeat_interleave(H // KV, dim=2))
    assert ((p * dp).sum(-1) - ref["delta"]).abs().max().item() < 1e-10


def test_row_rel_err_floor():
    ref = torch.ones(1, 100, 1, 4)
    ref[0, 0] = 0.0     # an all-zero row: the floor is its denominator
    ref[0, 1] *= 0.01   # under 5 % of the median: floored too
    got = ref.clone()
    got[0, 0, 0, 0] = 0.05
    got[0, 5, 0, 0] += 0.2
    e, share = A.row_rel_err(got, ref)
    assert share == pytest.approx(0.02)
    assert e[0, 0, 0].item() == pytest.approx(0.05 / (0.05 * 2.0))
    assert e[0, 5, 0].item() == pytest.approx(0.2 / 2.0)
    assert e[0, 2, 0].item() == 0.0


def test_tolerances_are_three_times_emulation(measured):
    """Prints the table that TOL was taken from and holds TOL to it: each bound
    is 3 x the group's worst emulation error, rounded up to one significant
    digit.  (The fp32 sums of the emulation may differ in the last bits from
    one BLAS to the next, so a bound may sit one rounding step away: the worst
    value is given 10 % either way.)"""
    worst = {}
    print()
    print(f"{'case':28s} " + " ".join(f"{n:8s}" for n in KEYS))
    for cid, (c, _, _, e) in measured.items():
        use = A.bounded(c)
        print(f"{cid:28s} " + " ".join(f"{e[n]:.2e}" if n in use else "   -    " for n in KEYS))
        w = worst.setdefault(c.group, {})
        for n in use:
            w[n] = max(w.get(n, 0.0), e[n])
    for g, w in worst.items():
        print(f"{g + ' worst':28s} " + " ".join(f"{w[n]:.2e}" if n in w else "   -    " for n in KEYS))
        print(f"{g + ' bound':28s} " + " ".join(f"{A.TOL[g][n]:<8.0e}" if n in w else "   -    " for n in KEYS))
    assert set(worst) == set(A.TOL)
    for g, w in worst.items():
        assert set(w) == set(A.TOL[g]), g
        for n, x in w.items():
            lo, hi = A.round_up_1sig(3 * x * 0.9), A.round_up_1sig(3 * x * 1.1)
            assert lo * (1 - 1e-9) <= A.TOL[g][n] <= hi * (1 + 1e-9), \
                f"{g} {n}: bound {A.TOL[g][n]:.0e}, 3 x emulation worst = {3 * x:.3e}"


def test_inputs_meet_conditions(measured):
    """With the reference alone: at most 2 % of the rows of any bounded
    quantity sit under the floor, and no row of o is all-zero."""
    for cid, (c, _, ref, _) in measured.items():
        share = A.floored_share(ref)
        for n in A.ROW_QUANTITIES:
            if n in A.bounded(c):
                assert share[n] <= FLOORED_CAP, f"{cid} {n}: {100 * share[n]:.2f} % of the rows floored"
        assert (ref["o"].norm(dim=-1) > 0).all(), cid


def _uniform_cases():
    return [(1, 384, 2, 1, 41), (2, 256, 8, 4, 42)]


@pytest.mark.parametrize("B,S,H,KV,seed", _uniform_cases())
def test_uniform_inputs_expected(B, S, H, KV, seed):
    q, k, v = A.uniform_inputs(B, S, H, KV, seed)
    assert v.float().abs().max() <= 4 and torch.equal(v.float(), v.float().round())
    o, lse2 = A.ref64(q, k, v, A.DEFAULT_SCALE)
    eo, el = A.uniform_expected(v, H)
    assert (o - eo).abs().max().item() < 1e-12
    assert (lse2 - el).abs().max().item() < 1e-12
    assert (eo.norm(dim=-1) > 0).all()


@pytest.mark.parametrize("case", A.RAMPS, ids=lambda c: c.id)
def test_ramp_realised_slope(case):
    """From the actual bf16 inputs: over the key tiles wholly below a row's
    diagonal, the tile maximum of head 0's scaled base-2 scores moves by the
    nominal slope per tile, within 0.5 (for a positive slope that is the rise
    of the row's running max; for a negative one the running max stays where
    tile 0 put it and the tile maxima fall).  Head 1: -slope / 2."""
    q, k, _, _ = A.build(case)
    S, slope = case.shape[1], case.scale
    z2 = torch.einsum("ihd,jd->hij", q[0].double(), k[0, :, 0].double()) * A.DEFAULT_SCALE * A.LOG2E
    tmax = z2.view(2, S, S // 64, 64).amax(-1)                # [head, row, tile]
    rise = tmax[:, :, 1:] - tmax[:, :, :-1]
    rows, tiles = torch.arange(S)[:, None], torch.arange(1, S // 64)[None, :]
    full = (64 * tiles + 63 <= rows).expand(2, -1, -1)        # both tiles wholly causal
    for h, nominal in ((0, slope), (1, -slope / 2)):
        r = rise[h][full[h]]
        assert r.numel() > 0
        assert (r - nominal).abs().max().item() <= 0.5, (h, r.min().item(), r.max().item())
    if slope > 0:
        # the running max itself, row S-1 of head 0: crosses the deferral
        # threshold of 8 log2 units every ceil(8 / slope)-th tile at the earliest
        run = tmax[0, S - 1].cummax(0).values
        assert ((run[1:] - run[:-1]) - slope).abs().max().item() <= 0.5
    else:
        run = tmax[0, S - 1]
        assert run[0] == run.max() and (run[0] - run[-1]).item() > 16  # later p underflow toward 0


@pytest.mark.parametrize("case", A.SM_SCALES, ids=lambda c: c.id)
def test_wrong_sm_scale_violates_bounds(case, measured):
    """A kernel that ignored sm_scale (ran at the default), or applied it to
    only one of dQ and dK, misses a bound of every quantity it touches by 10 x
    or more on these inputs.  (For dQ that bound is the q90 one: a relative
    error cannot exceed its loose worst-row bound tenfold.)"""
    c, (q, k, v, do), ref, _ = measured[case.group + " " + case.id]
    tol = A.TOL[case.group]

    def excess(e, n):
        return max(e[m] / tol[m] for m in (n, n + "_q90") if m in e)

    wrong = A.ref64_all(q, k, v, do, A.DEFAULT_SCALE)
    e = A.errors(wrong, ref)
    for n in ("o", "dq", "dk", "dv", "lse2"):
        print(f"{case.id} at the default scale, {n}: {excess(e, n):.1f} x its bound")
        assert excess(e, n) >= 10, f"{n}: {e}"
    ratio = A.DEFAULT_SCALE / case.sm_scale
    for n in ("dq", "dk"):      # the right softmax, the constant in the final factor only
        e = A.errors({n: ref[n] * ratio}, ref)
        print(f"{case.id} constant factor on {n} only: {excess(e, n):.1f} x its bound")
        assert excess(e, n) >= 10, f"{n}: {e}"
