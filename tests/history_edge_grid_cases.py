"""The corner images of tests/history_edge_cases.py for the six queries merged
after it: fold, joint, corr, period, shifts and match.  Images 1 to 9 are
reused as they are, one set of arguments per distinct (ring, t0, t1); four
images are added for the cell grid of period, shifts and match, whose edges
the bucket images put no slot on.  The host twins
(tests/test_history_edge_grid_cpu.py) and the kernels
(tests/test_history_edge_grid_gpu.py) are held to each query's own assert_same
against the NumPy references of dynolog_amd.utils.slots on images 1 to 9 and
the cell images, and to invariants on image 10.

The arguments.  metric hbm_read_gbps (every pass carries it); a grid of about
1000 cells, cell_ns = ceil((t1 - t0) / 1000); max_lag 40, window 20, min_n 1; a
template of 32 cells from cell G // 10, min_fill 0.1, min_r 0.5; corr with
min(B, 64) buckets and the automatic centre; joint with
history_joint_cases.DEFAULTS; fold with history_fold_cases.ANCHOR_IDS and
DEFAULTS.  On the 10 ms windows of the equal_ts rings and on edge_exact_B7 a
second grid of 2 * 2048 + 3 cells (cell_ns = ceil(w / 4099)) crosses the period
chunk and the scan chunk and gives match 4068 positions, above its tile.

The cell images.  cell_edge_exact: w = 1 000 003, cell_ns = 142 857 = floor(w /
7), so that G = 8 and the last cell is 4 ns long (142 858 = ceil(w / 7) gives
seven cells, and a max_lag of 7 would be refused); a slot at every cell edge -
1, edge, edge + 1, at t1 - 1 and at t1.  cell_collisions: the equal_ts rings at
one cell per run (G = 10) and at 250 us (G = 40); in cell_collisions_torn_winner
the last slot of the run of 130, the one that would win its cell, is torn in
the high word of its seq only.  widest_grid: the widest window at cell_ns =
2^31, G = 2^20.  t0_zero at 1 ms cells.

Special values.  The fp64 sums of fold and joint are held to the summation
bound of history_edge_cases (2 n 2^-53 sum|term|, sum|term| from the same
reference on abs_ring, n the reference's count) where their own rtol 1e-9 is
not valid.  Period and match get a given centre there.  The automatic centre is
float32(wsum / w); where terms of wsum cancel, two summation orders differ by
up to 2 n 2^-53 sum|term| (the same bound), which on that ring is more than the
centre itself: one float32 ulp, which history_period_cases.assert_same asks of
the automatic centre, holds between two orders only where the terms have one
sign.  For the same reason check_corr_special holds the automatic centre on the
copy of the ring to CENTER_BOUND: ulp(c) + 2 n 2^-53 (sum|v dt| / w + |c|), the
first term the rounding to float32, the second the two sums' orders (wsum by
the bound above, w, all positive, by 2 n 2^-53 w, that is 2 n 2^-53 |c| of the
quotient).  The records are then taken at the answer's own centre, as
history_corr_cases.assert_same does.  The derived corr of a pair is var = q / w
- (s / w)^2 and the like: differences of numbers of the size (mean - c)^2,
each carrying n 2^-53 of itself in rounding.  On the copy one metric's centre
is the window's mean, about 1e16 because of the +-2^60 it holds somewhere,
while a bucket's pair without such a value has a variance of about 1e3 about
a mean of about 50: off = (mean - c)^2 / var is 1e29 there, and no fp64 sum
about that centre says whether the variance is positive.  That is a property
of the record format, the same for kernel, twin and the NumPy derive.  So a
corr is owed only where 64 n 2^-53 (1 + off) < 1, the bound of
history_corr_cases.assert_same staying below 1, with off from the two-pass
reference and not from the answer (`resolvable`); there it is held to that
bound.  The CPU file asserts how many pairs that leaves.

A ring out of time order (image 10, check_out_of_order).  The range search runs
on keys that are not sorted, so [seq_begin, seq_end) is some sub-range of
[seq_lo, seq_hi): lo <= seq_begin <= seq_end <= hi.  Inside it every
implementation classes each position once, by the slot's own fields
(dynoHistoryJointClass): the class counts add up to no more than seq_end -
seq_begin.  For the grid queries these are n_eligible + n_not_carried +
n_not_finite + stale; for joint the same; for corr the buckets' n_slots +
stale, with n_used <= n_slots and n[i][j] <= n_used per bucket; for fold
n_folded + n_beyond + n_misplaced + n_outside + stale.  An eligible slot
passed ts < t1 itself, so its cell is below G whatever the order: it fills a
cell or collides, n_filled + n_collided == n_eligible and n_filled <= cells.  A
lag's or a position's pairs are pairs of filled cells: n <= n_filled (a
position's also <= tpl_filled).  Lists are cut at `returned`, in ascending
order of cell (shifts, match) or first_seq (fold), inside the window or range,
and nothing past `returned` is written.  No sum is a floating-point atomic:
two runs give the same bytes.  The answers are not compared with the host
twin's or the reference's: the two searches probe different positions.
"""
import functools

import numpy as np

import history_corr_cases as HC
import history_edge_cases as E
import history_fold_cases as HF
import history_joint_cases as HJ
import history_match_cases as HM
import history_period_cases as HPd
import history_shift_cases as HS
from dynolog_amd.utils import slots as S

HBM, DT, MS, REAL = E.HBM, E.DT, E.MS, E.REAL
SPECIAL = "special_values_B3"
GIVEN_CENTER = 33.25  # period and match on SPECIAL (module docstring)
CORR_RUNS = 16        # kCorrRuns of kernels/history.hip: runs of partials per bucket in the corr combine
SECOND_GRID = 2 * HPd.CHUNK + 3


# ---- the images ----------------------------------------------------------

def _eligible_but_for_seq(ring, pos):
    x = ring[pos]
    dt = x["derived"][DT]
    return bool((x["flags"] & S.SLOT_FIRST) == 0 and np.isfinite(dt) and dt > 0 and np.isfinite(x["derived"][HBM]))


@functools.lru_cache(maxsize=None)
def new_windows():
    """The rings of the cell images that images 1 to 9 do not hold, as windows
    (id, ring, ring_slots, seq_lo, seq_hi, t0, t1, B)."""
    out = []
    # cell_edge_exact: every slot usable (main pass, no flags, an interval), the values make_ring's
    lo, t0, w, cell = 2**40 + 5, REAL + 11, 1_000_003, 142_857
    G = S.history_period_cells(t0, t0 + w, cell)
    assert G == 8 and w - 7 * cell == 4
    ts = np.array(sorted({t0 + g * cell + k for g in range(G) for k in (-1, 0, 1)} | {t0 + w - 1, t0 + w}), dtype=np.int64)
    assert len(ts) == 26
    ring = E.H.make_ring(64, lo, ts, 58)
    pos = (np.arange(lo, lo + len(ts)) & 63).astype(np.int64)
    ring["flags"][pos], ring["pass"][pos] = 0, S.PASS_MAIN
    ring["derived"][pos, DT] = 1000.0
    out.append(("cell_edge_exact", ring, 64, lo, lo + len(ts), t0, t0 + w, 1))
    # cell_collisions_torn_winner: the last slot of the run of 130 loses its seq's high word
    _, ring, ring_slots, lo, hi, t0, t1, _ = E.case("equal_ts_B10")
    _, runs = E.equal_ts_stamps()
    last = lo + int(np.cumsum(runs)[5]) - 1
    assert runs[5] == 130 and last >= 2**32 and _eligible_but_for_seq(ring, last & (ring_slots - 1))
    torn = ring.copy()
    torn["seq"][last & (ring_slots - 1)] = last - 2**32
    out.append(("cell_collisions_torn_winner", torn, ring_slots, lo, hi, t0, t1, 1))
    for c in out:
        c[1].flags.writeable = False
    return tuple(out)


def windows():
    """Images 1 to 9, one case of every (ring, t0, t1)."""
    return E.episode_cases()


def window(label):
    return {c[0]: c for c in tuple(windows()) + new_windows()}[label]


def _grid(label, c, cell_ns, max_lag=40, window=20, tpl_cell=None, tpl_cells=32, match=True):
    """One set of grid arguments on window c, cut down to what a grid of G cells takes."""
    _, ring, ring_slots, lo, hi, t0, t1, _ = c
    G = S.history_period_cells(t0, t1, cell_ns)
    a = G // 10 if tpl_cell is None else tpl_cell
    m = min(tpl_cells, G - a - 1)  # the last cell may be short: the template ends before it
    assert G >= 8 and m >= S.HISTORY_MATCH_MIN_CELLS and t0 + (a + m) * cell_ns <= t1, (label, G, a, m)
    return dict(label=label, image=c[0], ring=ring, ring_slots=ring_slots, lo=lo, hi=hi, t0=t0, t1=t1, cell_ns=cell_ns, G=G,
                max_lag=min(max_lag, G - 1), window=min(window, G - 1), tpl_cell=a, tpl_cells=m, match=match,
                center=GIVEN_CENTER if c[0] == SPECIAL else None)


@functools.lru_cache(maxsize=None)
def grids():
    """Every set of grid arguments (module docstring), as dicts."""
    out = []
    for c in windows():
        w = c[6] - c[5]
        out.append(_grid(f"{c[0]}/G1000", c, -(-w // 1000)))
    second = [c for c in windows() if c[0] in ("equal_ts_B1", "equal_ts_torn_by_high_word_B10", "edge_exact_B7")]
    assert len(second) == 3
    for c in second:
        g = _grid(f"{c[0]}/G{SECOND_GRID}", c, -(-(c[6] - c[5]) // SECOND_GRID))
        assert g["G"] == SECOND_GRID
        out.append(g)
    out.append(_grid("cell_edge_exact/G8", window("cell_edge_exact"), 142_857, max_lag=7, window=2, tpl_cell=2, tpl_cells=4))
    for name, src in (("cell_collisions_equal_ts", "equal_ts_B1"), ("cell_collisions_torn_by_high_word", "equal_ts_torn_by_high_word_B10"),
                      ("cell_collisions_torn_winner", "cell_collisions_torn_winner")):
        for cell in (MS, MS // 4):
            g = _grid(f"{name}/G{10 * MS // cell}", window(src), cell)
            assert g["G"] == 10 * MS // cell
            out.append(g)
    # match is left out at G = 2^20: its yardstick walks the 2^20 positions one by one in Python (minutes); the
    # widest window runs through match at G = 1000 above
    g = _grid("widest_grid/G1048576", window("widest_window_B4096"), 2**31, max_lag=16, window=5000, match=False)
    assert g["G"] == S.HISTORY_PERIOD_MAX_CELLS
    out.append(g)
    out.append(_grid("t0_zero/1ms", window("t0_zero_B2"), MS))
    assert len({g["label"] for g in out}) == len(out)
    return tuple(out)


def grid(label):
    return {g["label"]: g for g in grids()}[label]


def match_grids():
    return [g for g in grids() if g["match"]]


def _head(g):
    return g["label"], g["ring"], g["ring_slots"], g["lo"], g["hi"], g["t0"], g["t1"]


def period_case(g):
    return _head(g) + (dict(metric=HBM, cell_ns=g["cell_ns"], max_lag=g["max_lag"], center=g["center"], phase=None),)


def shift_case(g):
    return _head(g) + (dict(metric=HBM, cell_ns=g["cell_ns"], window=g["window"], min_n=1, min_delta=0.0, max_shifts=16,
                            phase=None),)


def match_case(g):
    a = g["t0"] + g["tpl_cell"] * g["cell_ns"]
    return _head(g) + (dict(metric=HBM, cell_ns=g["cell_ns"], tpl_t0_ns=a, tpl_t1_ns=a + g["tpl_cells"] * g["cell_ns"], min_r=0.5,
                            min_fill=0.1, max_matches=16, center=g["center"], phase=None),)


def fold_case(c):
    return c[:7] + (list(HF.ANCHOR_IDS), dict(HF.DEFAULTS))


def joint_case(c):
    return c[:7] + (dict(HJ.DEFAULTS),)


def corr_case(c, center=None, label=None, ring=None):
    return (label or c[0], c[1] if ring is None else ring) + c[2:7] + (dict(buckets=min(c[7], 64), center=center, phase=None),)


@functools.lru_cache(maxsize=None)
def corr_special_copy():
    """special_values with +-FLT_MAX replaced by +-2^60 in every metric, the interval (whose own centre would be
    FLT_MAX otherwise) included."""
    ring = window(SPECIAL)[1].copy()
    n = window(SPECIAL)[4]
    bits = ring["derived"][:n].view(np.uint32)
    big = (bits & np.uint32(0x7FFFFFFF)) == np.uint32(E.F32_MAX_BITS)
    assert big[:, DT].any() and big[:, HBM].any()
    bits[big] = (bits[big] & np.uint32(0x80000000)) | np.float32(2.0**60).view(np.uint32)
    ring.flags.writeable = False
    return ring


# ---- the references, each computed once ----------------------------------

@functools.lru_cache(maxsize=None)
def fold_reference(label):
    """(reference, its records on the ring of magnitudes)."""
    case = fold_case(window(label))
    return HF.reference(case), HF.reference(case[:1] + (E.abs_ring(case[1]),) + case[2:])[2]


@functools.lru_cache(maxsize=None)
def joint_reference(label):
    case = joint_case(window(label))
    return HJ.reference(case), HJ.reference(case[:1] + (E.abs_ring(case[1]),) + case[2:])[1]


# ---- checks --------------------------------------------------------------

def _same_bytes(a, b):
    return a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def _fold_against(got, ref, ref_abs, label):
    """history_fold_cases.assert_same with the sums held to the summation bound."""
    ref_hdr, ref_fh, ref_out, ref_per = ref
    listed = np.full(len(got[5]) * 32, 0xEE, dtype=np.uint8).view(S.HISTORY_PERIOD_DTYPE)
    listed[:len(ref_per)] = ref_per
    HF.assert_same_exact_fields(got, (0, ref_hdr, ref_fh, ref_out, None, listed), label)
    E.assert_sums_within_bound(got[3], ref_out, ref_abs, label)
    assert (got[4].view(np.uint8) == 0xEE).all(), f"{label}: a record past `bins` was written"


def check_fold(lib, c, use_host, twin=False):
    label = c[0]
    case = fold_case(c)
    ref, ref_abs = fold_reference(label)
    got = HF.run_case(lib, case, use_host=use_host)
    if label == SPECIAL:
        _fold_against(got, ref, ref_abs, label)
    else:
        HF.assert_same(got, ref, label)
    if twin:
        assert _same_bytes(HF.run_case(lib, case, use_host=use_host), got), label
        HF.assert_same_exact_fields(got, HF.run_case(lib, case, use_host=1), f"{label} twin")


def joint_bounds(ref_jh, ref_abs_jh):
    n = float(ref_jh["n_eligible"])
    return {f: 2.0 * n * E.U * float(ref_abs_jh[f]) for f in HJ.MOMENTS}


def check_joint(lib, c, use_host, twin=False):
    label = c[0]
    case = joint_case(c)
    ref, ref_abs_jh = joint_reference(label)
    got = HJ.run_case(lib, case, use_host=use_host)
    if label == SPECIAL:
        HJ.assert_same_exact(got, ref, label)
        for f, bound in joint_bounds(ref[1], ref_abs_jh).items():
            err = abs(float(got[2][f]) - float(ref[1][f]))
            assert err <= bound, (label, f, float(got[2][f]), float(ref[1][f]), err, bound)
    else:
        HJ.assert_same(got, ref, label)
    if twin:
        assert _same_bytes(HJ.run_case(lib, case, use_host=use_host), got), label
        host = HJ.run_case(lib, case, use_host=1)
        (HJ.assert_same_exact if label == SPECIAL else HJ.assert_same)(got, host[1:4], f"{label} twin")


def center_bound(case):
    """CENTER_BOUND of the module docstring, per metric, from the plain reference at one bucket."""
    _, ring, ring_slots, lo, hi, t0, t1, _ = case
    _, whole = S.history_reference(ring, lo, hi, ring_slots, t0, t1, 1)
    _, mag = S.history_reference(E.abs_ring(ring), lo, hi, ring_slots, t0, t1, 1)
    auto = HC.reference(case, None)[1]["center"]
    n, w = whole["n"][0].astype(np.float64), whole["w"][0]
    with np.errstate(all="ignore"):
        spread = np.where(w > 0, mag["wsum"][0] / np.where(w > 0, w, 1.0), 0.0)
    return auto, np.spacing(np.abs(auto)).astype(np.float64) + 2.0 * n * E.U * (spread + np.abs(auto.astype(np.float64)))


def check_corr_special(lib, c, use_host):
    """-> the two answers.  The records on the full ring at a given centre; the automatic centre and the derived
    corr on the copy without +-FLT_MAX (module docstring)."""
    raw_case = corr_case(c, center=HC.GIVEN, label=f"{c[0]}/given")
    raw = HC.run_case(lib, raw_case, use_host=use_host)
    HC.assert_center(raw, raw_case)
    HC.assert_raw(raw, raw_case)
    copy_case = corr_case(c, label=f"{c[0]}/copy", ring=corr_special_copy())
    got = HC.run_case(lib, copy_case, use_host=use_host)
    assert got[0] == 0, (copy_case[0], got[0])
    auto, bound = center_bound(copy_case)
    err = np.abs(got[2]["center"].astype(np.float64) - auto.astype(np.float64))
    assert (err <= bound).all(), (copy_case[0], got[2]["center"], auto, bound)
    HC.assert_raw(got, copy_case)
    assert_derived_where_resolvable(got, copy_case)
    return raw, got


def resolvable(case, center):
    """-> (ok [buckets, 16, 16], off, two): the pairs whose two-pass corr exists and whose variances fp64 sums
    about `center` can resolve (module docstring), and (mean - c)^2 / var of the worse side, from the reference alone."""
    _, _, ref, _, two = HC.reference(case, center)
    c = np.asarray(center, dtype=np.float64)[None, :, None]
    with np.errstate(all="ignore"):
        off = ((two["mean"] - c) ** 2 / two["var"]).astype(np.float64)
    off = np.maximum(off, off.transpose(0, 2, 1))
    n = ref["n"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(two["corr"].astype(np.float64)) & (64 * n * 2.0**-53 * (1 + off) < 1)
    return ok, off, two


def assert_derived_where_resolvable(got, case):
    """history_corr_cases.assert_derived, its bound taken from the reference: a pair without samples or with a
    single one has no corr; a resolvable pair has one, within 64 n 2^-53 (1 + off) of the two-pass one."""
    label = case[0]
    rc, hdr, ch, recs, past = got
    ok, off, two = resolvable(case, ch["center"])
    for b in range(len(recs)):
        _, _, _, corr = S.history_corr_derive(recs[b], ch["center"])
        assert np.isnan(corr[recs[b]["n"] < 2]).all(), (label, b)
        want = two["corr"][b].astype(np.float64)
        err = np.where(ok[b], np.abs(corr - np.where(ok[b], want, 0.0)), 0.0)  # NaN where an answer has no corr
        bound = 64 * recs[b]["n"].astype(np.float64) * 2.0**-53 * (1 + np.where(ok[b], off[b], 0.0))
        bad = ok[b] & ~(err <= bound)
        assert not bad.any(), (label, b, np.argwhere(bad)[:4], err[bad][:4], bound[bad][:4])


def check_corr(lib, c, use_host, twin=False):
    if c[0] == SPECIAL:
        answers = check_corr_special(lib, c, use_host)
        if twin:
            again = check_corr_special(lib, c, use_host)
            assert all(_same_bytes(a, b) for a, b in zip(answers, again)), c[0]
            check_corr_special(lib, c, 1)
        return
    case = corr_case(c)
    got = HC.run_case(lib, case, use_host=use_host)
    HC.assert_same(got, case)
    if twin:
        assert _same_bytes(HC.run_case(lib, case, use_host=use_host), got), c[0]
        HC.assert_same(HC.run_case(lib, case, use_host=1), case)


def check_period(lib, g, use_host, twin=False):
    case = period_case(g)
    got = HPd.run_case(lib, case, use_host=use_host)
    HPd.assert_same(got, case)
    if twin:
        assert _same_bytes(HPd.run_case(lib, case, use_host=use_host), got), g["label"]
        HPd.assert_same(HPd.run_case(lib, case, use_host=1), case)


def check_shifts(lib, g, use_host, twin=False):
    case = shift_case(g)
    got = HS.run_case(lib, case, use_host=use_host)
    HS.assert_same(got, case)
    if twin:
        assert _same_bytes(HS.run_case(lib, case, use_host=use_host), got), g["label"]
        assert _same_bytes(HS.run_case(lib, case, use_host=1), got), f"{g['label']} twin"  # every field is exact


def check_match(lib, g, use_host, twin=False):
    case = match_case(g)
    got = HM.run_case(lib, case, use_host=use_host)
    HM.assert_same(got, case)
    if twin:
        assert _same_bytes(HM.run_case(lib, case, use_host=use_host), got), g["label"]
        HM.assert_same(HM.run_case(lib, case, use_host=1), case)


# ---- a second yardstick for the cell grid: every slot by its own stamp ---

GRID_MUTANTS = ("lowest_position_wins", "cell_index_rounds_to_nearest", "t1_inclusive", "seq_high_word_dropped",
                "last_cell_dropped_when_short", "value_bits_zero_means_empty")


def direct_grid(g, mutant=None):
    """Per cell the winner as the argmax over the eligible slots of (position,
    value bits), every slot placed by its own stamp, no range search ->
    dict(n_eligible, n_filled, n_collided, lag_n[max_lag + 1], filled[G],
    bits[G], later_slot_wins: the cells of several slots that another than the
    first of them won).  `mutant`: one of GRID_MUTANTS, a wrong reading of the
    definition."""
    ring, ring_slots, lo, hi, t0, t1, cell_ns, G = (g[k] for k in ("ring", "ring_slots", "lo", "hi", "t0", "t1", "cell_ns", "G"))
    seqs = np.arange(lo, hi, dtype=np.uint64)
    x = ring[(seqs & np.uint64(ring_slots - 1)).astype(np.int64)]
    ts = x["host_ts_ns"]
    low = np.uint64(0xFFFFFFFF)
    same = (x["seq"] & low) == (seqs & low) if mutant == "seq_high_word_dropped" else x["seq"] == seqs
    inside = (ts >= np.uint64(t0)) & ((ts <= np.uint64(t1)) if mutant == "t1_inclusive" else (ts < np.uint64(t1)))
    dtf, v = x["derived"][:, DT], x["derived"][:, HBM]
    with np.errstate(invalid="ignore"):
        ok = (same & inside & ((x["flags"] & S.SLOT_FIRST) == 0) & np.isfinite(dtf) & (dtf > 0)
              & (((S.derived_mask(x["pass"]) >> HBM) & 1) == 1) & np.isfinite(v))
    off = ts[ok] - np.uint64(t0)
    cell = (2 * off + np.uint64(cell_ns)) // np.uint64(2 * cell_ns) if mutant == "cell_index_rounds_to_nearest" else off // np.uint64(cell_ns)
    cells = (t1 - t0) // cell_ns if mutant == "last_cell_dropped_when_short" else G
    cell = cell.astype(np.int64)
    if mutant == "last_cell_dropped_when_short":
        keep = cell < cells
    else:
        cell, keep = np.minimum(cell, G - 1), np.ones(len(cell), dtype=bool)
    pos = (seqs[ok] - np.uint64(lo) + np.uint64(1))[keep]
    bits = np.ascontiguousarray(v[ok]).view(np.uint32)[keep].astype(np.uint64)
    cell = cell[keep]
    word = (pos << np.uint64(32)) | bits
    if mutant == "lowest_position_wins":
        best = np.full(G, np.iinfo(np.uint64).max, dtype=np.uint64)
        np.minimum.at(best, cell, word)
        best[best == np.iinfo(np.uint64).max] = 0
    else:
        best = np.zeros(G, dtype=np.uint64)
        np.maximum.at(best, cell, word)
    filled = (best & low) != 0 if mutant == "value_bits_zero_means_empty" else best != 0
    first = np.full(G, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(first, cell, pos)
    many = np.bincount(cell, minlength=G) > 1
    n_filled = int(np.count_nonzero(filled))
    return dict(n_eligible=len(cell), n_filled=n_filled, n_collided=len(cell) - n_filled,
                lag_n=np.array([np.count_nonzero(filled[:G - l] & filled[l:]) for l in range(g["max_lag"] + 1)], dtype=np.uint64),
                filled=filled, bits=(best & low).astype(np.uint32),
                later_slot_wins=int(np.count_nonzero(many & filled & ((best >> np.uint64(32)) != first))))


@functools.lru_cache(maxsize=None)
def _shift_reference(label):
    return HS.reference(shift_case(grid(label)))


SHIFT_GRID_FIELDS = ("n_filled", "n_clamped", "n_valid", "n_shifts", "n_up", "n_down", "returned", "strongest_cell",
                     "strongest_delta")


def direct_grid_agrees(g, mutant=None):
    """n_eligible, n_filled, n_collided and every lag's n against the period
    reference; the winners' values through the shift reference: one usable slot
    per filled cell, at the cell's start and with the winner's value, must give
    the shift header and records of the ring itself."""
    d = direct_grid(g, mutant)
    _, ph, recs, _ = HPd.reference(period_case(g), g["center"])
    if any(int(ph[f]) != d[f] for f in ("n_eligible", "n_filled", "n_collided")) or not np.array_equal(recs["n"], d["lag_n"]):
        return False
    at = np.flatnonzero(d["filled"])
    if len(at) == 0:
        return int(_shift_reference(g["label"])[1]["n_filled"]) == 0
    slots = 1 << max(6, int(len(at)).bit_length())
    ring = HPd.plain_ring(slots, np.uint64(g["t0"]) + at.astype(np.uint64) * np.uint64(g["cell_ns"]),
                          np.ascontiguousarray(d["bits"][at]).view(np.float32))
    kw = shift_case(g)[7]
    _, sh, out = S.history_shifts_reference(ring, 0, len(at), slots, g["t0"], g["t1"], **kw)
    _, ref_sh, ref_out = _shift_reference(g["label"])
    return all(sh[f].tobytes() == ref_sh[f].tobytes() for f in SHIFT_GRID_FIELDS) and out.tobytes() == ref_out.tobytes()


# ---- image 10: what holds for a ring out of time order -------------------

def _range_ok(hdr, lo, hi, label):
    begin, end = int(hdr["seq_begin"]), int(hdr["seq_end"])
    assert lo <= begin <= end <= hi, (label, begin, end)
    return begin, end


def _grid_header_ok(hdr, gh, lo, hi, G, label):
    begin, end = _range_ok(hdr, lo, hi, label)
    classes = int(gh["n_eligible"]) + int(gh["n_not_carried"]) + int(gh["n_not_finite"]) + int(hdr["stale"])
    assert classes <= end - begin, (label, classes, begin, end)
    assert int(gh["n_filled"]) + int(gh["n_collided"]) == int(gh["n_eligible"]), label
    assert int(gh["n_filled"]) <= G == int(gh["cells"]), label


def check_out_of_order(lib, c, use_host):
    """All six queries on image 10, one implementation on its own (module docstring)."""
    label, ring, ring_slots, lo, hi, t0, t1, B = c
    # fold
    case = fold_case(c)
    got = HF.run_case(lib, case, use_host=use_host)
    assert got[0] == 0, label
    _, hdr, fh, out, past, per = got
    begin, end = _range_ok(hdr, lo, hi, label)
    placed = sum(int(fh[f]) for f in ("n_folded", "n_beyond", "n_misplaced", "n_outside"))
    assert placed + int(hdr["stale"]) <= end - begin, (label, placed)
    assert int(out["n_slots"].sum()) == int(fh["n_folded"]) and (out["n"] <= out["n_slots"][:, None]).all(), label
    assert int(fh["n_kept"]) <= int(fh["n_periods"]) <= max(int(fh["n_entries"]) - 1, 0), label
    k = int(fh["returned"])
    assert k == min(int(fh["n_periods"]), case[8]["max_listed"]) and (per[k:].view(np.uint8) == 0xEE).all(), label
    assert (past.view(np.uint8) == 0xEE).all(), label
    p = per[:k]
    assert (p["first_seq"] >= begin).all() and (p["first_seq"] + p["n_slots"] <= end).all(), label
    assert (p["first_seq"][1:] >= (p["first_seq"] + p["n_slots"])[:-1]).all(), label
    assert ((p["start_ns"] >= t0) & (p["start_ns"] < t1)).all(), label
    assert _same_bytes(HF.run_case(lib, case, use_host=use_host), got), label
    # joint
    case = joint_case(c)
    got = HJ.run_case(lib, case, use_host=use_host)
    assert got[0] == 0, label
    _, hdr, jh, cells, past = got
    begin, end = _range_ok(hdr, lo, hi, label)
    assert int(jh["n_eligible"]) + int(jh["n_not_carried"]) + int(jh["n_not_finite"]) + int(hdr["stale"]) <= end - begin, label
    assert int(cells["n"].sum()) == int(jh["n_eligible"]) and int(cells["dt_ns"].sum()) == int(jh["covered_ns"]), label
    assert all(int(jh[f]) <= int(jh["n_eligible"]) for f in ("n_x_below", "n_x_above", "n_y_below", "n_y_above")), label
    assert (past.view(np.uint8) == 0xEE).all(), label
    assert _same_bytes(HJ.run_case(lib, case, use_host=use_host), got), label
    # corr
    case = corr_case(c)
    got = HC.run_case(lib, case, use_host=use_host)
    assert got[0] == 0, label
    _, hdr, ch, recs, past = got
    begin, end = _range_ok(hdr, lo, hi, label)
    assert int(recs["n_slots"].sum()) + int(hdr["stale"]) <= end - begin, label
    assert (recs["n_used"] <= recs["n_slots"]).all() and int(recs["n_used"].sum()) == int(ch["n_used"]), label
    assert (recs["n"] <= recs["n_used"][:, None, None]).all() and (recs["n"] == recs["n"].transpose(0, 2, 1)).all(), label
    first = recs["first_seq"][recs["n_slots"] > 0]
    assert ((first >= begin) & (first < end)).all(), label
    assert (past.view(np.uint8) == 0xEE).all(), label
    assert _same_bytes(HC.run_case(lib, case, use_host=use_host), got), label
    # the grid queries
    g = _grid(f"{label}/G1000", c, -(-(t1 - t0) // 1000))
    G = g["G"]
    case = period_case(g)
    got = HPd.run_case(lib, case, use_host=use_host)
    assert got[0] == 0, label
    _, hdr, ph, lags, past = got
    _grid_header_ok(hdr, ph, lo, hi, G, label)
    assert (lags["n"] <= int(ph["n_filled"])).all() and int(lags["n"][0]) == int(ph["n_filled"]), label
    assert (past.view(np.uint8) == 0xEE).all(), label
    assert _same_bytes(HPd.run_case(lib, case, use_host=use_host), got), label
    case = shift_case(g)
    got = HS.run_case(lib, case, use_host=use_host)
    assert got[0] == 0, label
    _, hdr, sh, recs = got
    _grid_header_ok(hdr, sh, lo, hi, G, label)
    assert int(sh["n_clamped"]) <= int(sh["n_filled"]) and int(sh["n_valid"]) < G, label
    assert int(sh["n_up"]) + int(sh["n_down"]) <= int(sh["n_shifts"]) <= int(sh["n_valid"]), label
    k = int(sh["returned"])
    assert k == min(int(sh["n_shifts"]), case[7]["max_shifts"]) and (recs[k:].view(np.uint8) == 0xEE).all(), label
    r = recs[:k]
    assert (np.diff(r["cell"].astype(np.int64)) > 0).all() and ((r["cell"] >= 1) & (r["cell"] < G)).all(), label
    assert (r["t_ns"] == np.uint64(t0) + r["cell"] * np.uint64(g["cell_ns"])).all() and (r["t_ns"] < t1).all(), label
    assert (r["n_before"] <= g["window"]).all() and (r["n_after"] <= g["window"]).all(), label
    assert _same_bytes(HS.run_case(lib, case, use_host=use_host), got), label
    case = match_case(g)
    got = HM.run_case(lib, case, use_host=use_host)
    assert got[0] == 0, label
    _, hdr, mh, recs, r, n, sums = got
    _grid_header_ok(hdr, mh, lo, hi, G, label)
    P = G - g["tpl_cells"] + 1
    assert len(n) == P and int(mh["tpl_filled"]) <= g["tpl_cells"], label
    assert (n <= min(int(mh["n_filled"]), int(mh["tpl_filled"]))).all() and (sums[:, 0] == n).all(), label
    k = int(mh["returned"])
    assert k == min(int(mh["n_matches"]), case[7]["max_matches"]) and (recs[k:].view(np.uint8) == 0xEE).all(), label
    assert int(mh["n_matches"]) <= int(mh["n_scored"]) <= P, label
    m = recs[:k]
    assert (np.diff(m["cell"].astype(np.int64)) > 0).all() and (m["cell"] < P).all(), label
    assert (m["n"] == n[m["cell"]]).all() and (m["r"].view(np.uint32) == r.view(np.uint32)[m["cell"]]).all(), label
    assert _same_bytes(HM.run_case(lib, case, use_host=use_host), got), label
