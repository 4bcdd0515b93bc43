"""The case table of the pack-kernel tests (tests/pack_cases.py) on the CPU: its
invariants, the host twin hostPack() against the float64 reference on every
reduction case, and the proof that the table and its bounds can tell a wrong
kernel from a right one (every deliberately wrong variant of the reference
falls outside the bounds on at least one case).  The same cases run through
the kernels in tests/test_pack_gpu.py."""
import numpy as np
import pytest

import pack_cases as PC
from dynolog_amd import _native
from dynolog_amd.utils import slots as S


@pytest.fixture(scope="module")
def lib(native_built):
    return _native.load_gpu_lib()


@pytest.mark.parametrize("case", PC.REDUCTIONS, ids=PC.REDUCTION_IDS)
def test_host_pack_matches_reference(lib, case):
    out = PC.host_pack(lib, case)
    ref = PC.reference(case)
    bad = PC.reduction_failures(out["delta"], out["derived"], out["flags"], ref)
    assert not bad, "\n".join(bad[:20])
    np.testing.assert_array_equal(out["pass"], case.pass_id)
    np.testing.assert_array_equal(out["n_records"], case.raw.shape[1])
    np.testing.assert_array_equal(out["host_ts_ns"], case.ts)
    np.testing.assert_array_equal(out["reserved"], 0)


def test_case_invariants():
    by_id = dict(zip(PC.REDUCTION_IDS, PC.REDUCTIONS))
    assert len(by_id) == len(PC.REDUCTIONS)
    for c in PC.REDUCTIONS:
        PC.check_invariants(c)
        assert 1 <= len(c.raw) <= 3
    R = {i: c.raw.shape[1] for i, c in by_id.items()}
    assert R["odd_R"] == 783 and R["R1"] == 1 and R["max_stride"] == 4096 and R["max_stride_odd"] == 4095
    # the tail element of an odd R is the unique, non-zero maximum of a counter whose max is used
    for cid in ("odd_R", "max_stride_odd"):
        c = by_id[cid]
        k = c.counter_of[-1]
        assert k == S.C["GRBM_COUNT"]
        prev = np.vstack([c.prev_raw[None], c.raw[:-1]])
        d = (c.raw - prev)[:, c.counter_of == k]
        last = (c.raw - prev)[:, -1]
        assert (last > 0).all() and ((d == last[:, None]).sum(axis=1) == 1).all() and (d.max(axis=1) == last).all()
    c = by_id["wave_edges"]
    assert len(c.counts) == S.MAX_COUNTERS and {1, 63, 64, 65, 127, 129, 0, 200} <= set(c.counts)
    assert c.counts[14] > 0 and c.counts[15] > 64
    assert by_id["mfma_pass"].pass_id == S.PASS_MFMA and by_id["mfma_pass"].counts == PC.MFMA_COUNTS
    # one backwards record in sample 1 only, on a second trip, reset_far's in a counter of wave 3
    for cid in ("reset_far", "reset_far_max"):
        c = by_id[cid]
        k, i = PC.RESET_RECORD[cid]
        back = np.diff(c.raw, axis=0) < 0
        assert back.sum() == 1 and back[0, i] and c.raw[0, i] >= c.prev_raw[i]
        assert list(c.perm[c.seg_start[k]:]).index(i) >= 64 and c.counter_of[i] == k
        d, _, fl = PC.reference(c)
        assert list(fl) == [0, S.SLOT_RESET, 0]
        others = np.delete(c.raw[1] - c.raw[0], i)[np.delete(c.counter_of, i) == k]
        assert d[1, k] == int(others.sum()) + int(c.raw[1, i]) and c.raw[1, i] > others.max()
    assert PC.RESET_RECORD["reset_far"][0] % 4 == 3
    # the time edges: interval 0, every rate exactly 0, busy still derived
    for cid in ("time_equal", "time_backwards"):
        c = by_id[cid]
        assert c.ts[1] == c.ts[0] if cid == "time_equal" else c.ts[1] < c.ts[0]
        der = PC.reference(c)[1][1]
        assert all(der[S.D[n]] == 0 for n in PC.RATES) and der[S.D["gpu_busy_pct"]] > 0 and der[S.D["mfma_util"]] > 0
    d, der, fl = PC.reference(by_id["none_first"])
    assert fl[0] == S.SLOT_FIRST and (der == 0).all() and (d[0, :14] > 0).all()
    assert PC.reference(by_id["big_sums"])[0].max() > 1.4 * 2**51
    d = PC.reference(by_id["sum_2p52_odd"])[0]
    for k, total in PC.ODD_SUMS.items():
        assert d[0, k] == total and total % 2 == 1 and 2**52 <= total < 2**53


def test_comparison_helper():
    ref = np.zeros(len(S.DERIVED))
    one = np.float32(1.0)
    ref[S.D["sclk_mhz"]] = 1.0
    ref[S.D["gpu_busy_pct"]] = 1.0
    got = ref.astype(np.float32)
    assert not PC.derived_failures(got, ref)
    got[S.D["sclk_mhz"]] = np.nextafter(one, np.float32(2))                                     # 1 ulp: allowed
    got[S.D["gpu_busy_pct"]] = np.nextafter(np.nextafter(one, np.float32(2)), np.float32(2))    # 2 ulps: allowed
    assert not PC.derived_failures(got, ref)
    assert PC.derived_distance(got, ref)[S.D["sclk_mhz"]] == 1.0
    got[S.D["sclk_mhz"]] = np.nextafter(got[S.D["sclk_mhz"]], np.float32(2))                    # 2 ulps of a 1-ulp metric
    assert len(PC.derived_failures(got, ref)) == 1
    got = ref.astype(np.float32)
    got[S.D["waves_per_us"]] = 1e-30                                                            # reference 0: exactly 0
    assert len(PC.derived_failures(got, ref)) == 1
    ref[S.D["fp32_active"]] = 1e-3          # no absolute term: 10 % off a small ratio is far outside
    got = ref.astype(np.float32)
    got[S.D["fp32_active"]] = 1.1e-3
    assert len(PC.derived_failures(got, ref)) == 1
    got[S.D["fp32_active"]] = np.nan
    assert len(PC.derived_failures(got, ref)) == 1


@pytest.mark.parametrize("name", PC.WRONG_REDUCTIONS)
def test_table_catches_a_wrong_reduction(name):
    wrong = PC.WRONG_REDUCTIONS[name]
    caught = [c.id for c in PC.REDUCTIONS if PC.reduction_failures(*wrong(c), PC.reference(c))]
    assert caught, name
    must = {"drop_last": "odd_R", "first_trip_only": "wave_edges", "sum_for_max": "reset_far_max",
            "sticky_reset": "reset_far", "round_half_up": "sum_2p52_odd"}[name]
    assert must in caught, (name, caught)
    if name in ("sticky_reset", "round_half_up"):  # nothing else in the table has a reset or a tie
        assert set(caught) <= {"reset_far", "reset_far_max", "sum_2p52_odd"}


def test_the_right_reference_passes_its_own_comparison():
    for c in PC.REDUCTIONS:
        d, der, fl = PC.reference(c)
        assert not PC.reduction_failures(d, der.astype(np.float32), fl, (d, der, fl))


def test_table_catches_a_copy_that_skips_word_15():
    """Every slot the copy cases move has sixteen distinct random words: a copy
    that leaves word 15 (or any other) behind differs from the expected bytes."""
    for word in (0, 7, 15):
        w = PC.WINDOWS[0]
        x = PC.window_inputs(w)
        good = PC.expected_window_payload(w, x["gh"], x["ring"], x["ring"])
        assert not np.array_equal(good, PC.expected_window_payload(w, x["gh"], x["ring"], x["ring"], skip_word=word))
        cid, ring_slots, written, cursor, cap = PC.GATHER_PREPS[2]
        ring = PC.random_ring(1, ring_slots)
        assert not np.array_equal(PC.expected_gather_prep(ring, written, cursor, cap)[0],
                                  PC.expected_gather_prep(ring, written, cursor, cap, skip_word=word)[0])
        recv, _ = PC.drain_input(3, 16, [5, 23, 16], 2)
        assert not np.array_equal(PC.expected_drain(recv, 3, 16)[0], PC.expected_drain(recv, 3, 16, skip_word=word)[0])


def test_window_cases_are_legal_and_cover_the_shapes():
    """Every window is one the launcher accepts and the agent can produce; the
    shapes of the fused gather are all there."""
    shapes = set()
    for w in PC.WINDOWS:
        for n in (w.stage_slots, w.ring_slots):
            assert n & (n - 1) == 0
        assert w.n_pack <= w.stage_slots - 1
        end = w.begin + w.n_pack
        if w.payload is None:
            shapes.add("no_payload_n_pack_0" if w.n_pack == 0 else "no_payload")
            continue
        assert w.count <= w.cap and w.first_seq + w.count <= end
        assert end - min(w.first_seq, w.begin) <= w.ring_slots  # the backlog is still in the ring
        back = max(min(w.first_seq + w.count, w.begin) - w.first_seq, 0)
        fresh = w.count - back
        mask = w.ring_slots - 1
        shapes.add(("backlog" if back else "no_backlog") + ("+fresh" if fresh else ""))
        if w.count == 0:
            shapes.add("count_0")
        if w.n_pack == 0:
            shapes.add("n_pack_0")
        if w.first_seq > w.begin:
            shapes.add("starts_inside_fresh")
        if back and (w.first_seq & mask) + back > w.ring_slots:
            shapes.add("backlog_wraps")
        if w.n_pack and (w.begin & mask) + w.n_pack > w.ring_slots:
            shapes.add("fresh_wraps")
        if back * 16 > 64 * 256:
            shapes.add("copy_blocks_grid_stride")
        if w.payload == "hbm":
            shapes.add("collective")
        x = PC.window_inputs(w)
        assert len(x["fresh"]) == w.n_pack and x["R"] % 2 == 1
        for c in x["fresh"].values():
            PC.check_invariants(c)
    assert shapes >= {"backlog+fresh", "no_backlog+fresh", "backlog", "count_0", "n_pack_0", "no_payload_n_pack_0",
                      "starts_inside_fresh", "backlog_wraps", "fresh_wraps", "copy_blocks_grid_stride", "collective"}


def test_copy_cases_cover_the_shapes():
    plans = {cid: S.plan_gather_range(written, cursor, cap, ring) for cid, ring, written, cursor, cap in PC.GATHER_PREPS}
    caps = {cid: cap for cid, _, _, _, cap in PC.GATHER_PREPS}
    assert plans["nothing_pending"][1] == 0
    assert plans["count_eq_cap"][1] == caps["count_eq_cap"] > 0
    first, n = plans["wrapped"][:2]
    assert (first & 63) + n > 64
    first, n = plans["grid_stride"][:2]
    assert n * 16 > 256 * 256 and n < caps["grid_stride"] and (first & 16383) + n > 16384
    drains = {cid: (world, cap, counts) for cid, world, cap, counts in PC.DRAINS}
    assert drains["world_64"][:2] == (64, 4) and drains["cap_0"][1] == 0
    assert any(n > cap for _, cap, counts in drains.values() if counts for n in counts)
    recv, counts = PC.drain_input(3, 16, [5, 23, 16], 2)
    out, used = PC.expected_drain(recv, 3, 16)
    assert used == 64 * 3 + (5 + 16 + 16) * S.SLOT_BYTES and (out[used:] == PC.FILL).all()
    per = S.parse_compact_drain(out, 3)
    assert [int(h["count"]) for h, _ in per] == [5, 16, 16]
