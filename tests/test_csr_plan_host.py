"""The cases and bars of tests/test_gpu_csr_plan.py have teeth: the case builders of tests/util.py put a long row at every seam of
the count scan (thread, wave, block, carry pass, a block that is not full), the numpy planner agrees with a plain loop, and a planner
with one step left out -- no cross-wave term, no block carry, no running base between the carry kernel's passes -- makes
sage_csr_mean's chunk and row kernels (emulated in numpy fp32, csr_mean_under_plan) miss the fp64 bars of the GPU tests on the same
data by a wide factor.  A planner whose offsets are all too large does NOT change a single bit when the item list is exactly as long
as the plan (every long row falls back to its row wave): only the comparison of off[] and carry[nb] with the numpy planner sees it."""
import numpy as np
import pytest

from util import (PLAN_CARRY, PLAN_CHUNK, PLAN_DEGREES, PLAN_IPT, PLAN_LONG_BIG, PLAN_LONG_SMALL, PLAN_N_BIG, PLAN_N_SMALL, PLAN_TILE,
                  PLAN_WAVE, csr_mean_under_plan, csr_plan_case, csr_plan_reference, csr_rows_reference, plan_item_cap,
                  plan_tight_max_edges)

DIM = 4
WIDE = 100.0                                           # a read of another row's partial misses the bar by at least this factor


@pytest.fixture(scope="module")
def small():
    rowptr, col, deg = csr_plan_case(PLAN_N_SMALL, PLAN_LONG_SMALL, seed=1)
    table = np.random.default_rng(11).standard_normal((PLAN_N_SMALL, DIM)).astype(np.float32)
    return rowptr, col, deg, table, PLAN_LONG_SMALL


@pytest.fixture(scope="module")
def big():
    rowptr, col, deg = csr_plan_case(PLAN_N_BIG, PLAN_LONG_BIG, seed=2, filler=1)
    table = np.random.default_rng(12).standard_normal((PLAN_N_BIG, DIM)).astype(np.float32)
    return rowptr, col, deg, table, PLAN_LONG_BIG


def test_the_long_rows_sit_on_the_seams_of_the_count_scan(small, big):
    thread, wave, block = (lambda r: r // PLAN_IPT), (lambda r: r // (PLAN_IPT * PLAN_WAVE)), (lambda r: r // PLAN_TILE)
    s = PLAN_LONG_SMALL
    assert (thread(7), thread(8)) == (0, 1) and (wave(511), wave(512)) == (0, 1) and (wave(1535), wave(1536)) == (2, 3)
    assert (block(2047), block(2048)) == (0, 1) and (block(4095), block(4096)) == (1, 2)
    assert s[-1] == PLAN_N_SMALL - 1 and PLAN_N_SMALL % PLAN_TILE != 0 and set((7, 8, 511, 512, 1535, 1536, 2047, 2048, 4095, 4096)) < set(s)
    b = PLAN_LONG_BIG
    assert -(-PLAN_N_BIG // PLAN_TILE) == PLAN_CARRY + 2 and PLAN_N_BIG % PLAN_TILE != 0
    assert block(b[0]) == 0 and block(b[1]) == PLAN_CARRY - 1 and b[1] + 1 == b[2] and block(b[2]) == PLAN_CARRY and b[3] == PLAN_N_BIG - 1
    for (rowptr, col, deg, _, long_rows), filler, n in ((small, 6, PLAN_N_SMALL), (big, 1, PLAN_N_BIG)):
        assert len(deg) == n and rowptr[0] == 0 and np.array_equal(np.diff(rowptr), deg) and len(col) == rowptr[-1]
        assert np.array_equal(np.nonzero(deg > PLAN_CHUNK)[0], long_rows)
        assert [int(deg[r]) for r in long_rows] == [PLAN_DEGREES[i % 4] for i in range(len(long_rows))]
        rest = np.delete(deg, long_rows)
        assert set(np.unique(rest).tolist()) == set(range(filler + 1)), "filler degrees 0..filler, zeros included"
        assert col.min() >= 0 and col.max() < n
        own_last_chunk = 0
        for r in long_rows:
            beside = [q for q in (r - 1, r + 1) if 0 <= q < n and q not in long_rows]
            assert beside and all(deg[q] == 0 for q in beside), f"no empty row beside long row {r}"
            last = col[rowptr[r] + (deg[r] - 1) // PLAN_CHUNK * PLAN_CHUNK:rowptr[r + 1]]
            assert not (col[rowptr[r]:rowptr[r + 1] - len(last)] == r).any()
            own_last_chunk += bool((last == r).any())
        assert 0 < own_last_chunk < len(long_rows), "some long rows hold their own node in their last chunk, some do not"
    assert 900_000 <= len(big[1]) <= 1_200_000


def test_the_numpy_planner_is_a_plain_prefix_sum(small, big):
    deg = small[2]
    chunks, off, total = csr_plan_reference(deg)
    run = 0
    for r in range(len(deg)):
        k = (int(deg[r]) + PLAN_CHUNK - 1) // PLAN_CHUNK if deg[r] > PLAN_CHUNK else 0
        assert chunks[r] == k and off[r] == run, r
        run += k
    assert total == run == 29
    chunks, off, total = csr_plan_reference(big[2])
    assert np.array_equal(off, np.cumsum(chunks) - chunks) and total == chunks.sum() == 11
    # degrees of every size class, at random: the emulation's tiling never shows in a faithful plan
    deg = np.random.default_rng(0).choice([0, 3, 512, 513, 5000], 3 * PLAN_TILE * 2 + 77)
    chunks, off, total = csr_plan_reference(deg)
    assert np.array_equal(off, np.cumsum(chunks) - chunks) and total == chunks.sum()


def _outputs(case, off, total, cap, self_loop, last_wins):
    rowptr, col, _, table, long_rows = case
    got = csr_mean_under_plan(rowptr, col, table, long_rows, off, total, cap, self_loop, last_wins)
    return np.stack([got[r] for r in long_rows])


def _ratios(case, got, self_loop):
    """max over the columns of |got - fp64| / bar for every long row, with the bar of the GPU test"""
    rowptr, col, _, table, long_rows = case
    key = (len(rowptr), self_loop)
    if key not in _REFS:                                                   # computed once per case, shared, left unchanged
        ref, bar, _ = csr_rows_reference(rowptr, col, table, self_loop=self_loop)
        _REFS[key] = ref[np.asarray(long_rows)], bar[np.asarray(long_rows)]
    ref, bar = _REFS[key]
    return (np.abs(got.astype(np.float64) - ref) / bar).max(1)


_REFS = {}


# which long rows a missing step sends to the wrong items
WRONG = {
    ("small", "no_cross_wave"): (512, 1535, 1536, 2047, 4095),           # rows past wave 0 of a block with long rows before them
    ("small", "no_block_carry"): (2048, 4095, 4096, PLAN_N_SMALL - 1),   # every long row past block 0
    ("big", "no_block_carry"): PLAN_LONG_BIG[1:],
    ("big", "no_pass_base"): PLAN_LONG_BIG,                               # carry[nb] = 0 as well: no item is summed at all
}


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("which,broken", sorted(WRONG))
def test_a_planner_with_a_step_left_out_misses_the_output_bars(small, big, which, broken, self_loop):
    case = small if which == "small" else big
    deg, long_rows = case[2], np.asarray(case[4])
    cap = plan_item_cap(len(deg), int(case[0][-1]))                       # max_edges = len(col), the default
    _, off, total = csr_plan_reference(deg)
    assert cap >= total
    right = _outputs(case, off, total, cap, self_loop, True)
    assert _ratios(case, right, self_loop).max() <= 1.0, "the faithful plan meets the bar"
    _, off_b, total_b = csr_plan_reference(deg, broken)
    wrong_rows = long_rows[off_b[long_rows] != off[long_rows]]
    if broken == "no_pass_base":
        assert total_b == 0 and set(PLAN_LONG_BIG[2:]) <= set(wrong_rows.tolist())
    else:
        assert set(wrong_rows.tolist()) == set(WRONG[(which, broken)])
    assert np.all(off_b[long_rows] <= off[long_rows]), "the offsets only shrink: every item index stays inside the workspace"
    hit = np.zeros(len(long_rows), dtype=bool)
    for last_wins in (True, False):                                        # either outcome of two rows claiming one item
        got = _outputs(case, off_b, total_b, cap, self_loop, last_wins)
        ratio = _ratios(case, got, self_loop)
        foreign = (got.view(np.int32) != right.view(np.int32)).any(1)    # the row read a partial that is not its own
        assert foreign.any() and np.all(ratio[foreign] > WIDE), (long_rows[foreign].tolist(), ratio[foreign].tolist())
        assert np.all(ratio[~foreign] <= 1.0)
        hit |= foreign
    assert set(WRONG[(which, broken)]) <= set(long_rows[hit].tolist()), "every row with a wrong offset comes out wrong in one of the two"


@pytest.mark.parametrize("which", ["small", "big"])
def test_offsets_that_are_too_large_change_no_bit_only_the_plan_check_sees_them(small, big, which):
    case = small if which == "small" else big
    deg, long_rows = case[2], np.asarray(case[4])
    chunks, off, total = csr_plan_reference(deg)
    _, off_b, total_b = csr_plan_reference(deg, "shifted")
    assert total_b == total and np.all(off_b[long_rows] == off[long_rows] + total)
    tight = plan_tight_max_edges(len(deg), total)
    cap = plan_item_cap(len(deg), tight)
    assert total <= cap < total + 2 and tight < case[0][-1]
    for self_loop in (False, True):
        right = _outputs(case, off, total, cap, self_loop, True)
        got = _outputs(case, off_b, total_b, cap, self_loop, True)           # no row fits: every one is summed by its row wave
        assert np.array_equal(got.view(np.int32), right.view(np.int32)), "the fall-back gives the same bits: no output test can see it"
        assert _ratios(case, got, self_loop).max() <= 1.0
    assert not np.array_equal(off_b[long_rows], off[long_rows]), "the plan check compares off[] with the numpy planner"
    # with room to spare the shifted rows fit, but their items lie past carry[nb] and are never summed: stale partials, a wide miss
    cap = plan_item_cap(len(deg), int(case[0][-1]))
    if cap >= 2 * total:
        got = _outputs(case, off_b, total_b, cap, False, True)
        assert _ratios(case, got, False).min() > WIDE
