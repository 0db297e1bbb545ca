"""The bar of tests/test_gpu_linear_act.py has teeth and is reachable: the numpy fp32 emulation of linear_act_kernel's accumulation
and masks (util.linear_act_emulate: 32-wide K panels, the concat seam at panel column ds, rows past the row count and columns past
K zeroed, k ascending with two terms per matrix instruction, in both rounding variants) on the very cases and data of that module.

The bar of a case is twice the worst figure of the two variants, so the faithful emulation meets it by construction; what this
module shows is that the figures are the 0.5 to 1.8 units the bar was argued from, that the bar stays below one eighth of the
smallest single term's share on every case (so no dropped or misplaced term can pass), and that each broken emulation misses the
bar on every case it applies to.  No GPU and no library call.
"""
import numpy as np
import pytest

from util import (LINEAR_BROKEN, LINEAR_MODES, LINEAR_RUNS, LINEAR_SHAPES, LINEAR_VARIANTS, contraction_units, linear_act_emulate,
                  linear_bar, linear_broken_applies, linear_case, linear_n_devs, linear_operands, linear_poisoned)


def _id(run):
    n, dim, h, mode, small = run
    return f"n{n}-d{dim}-h{h}-{mode}"


@pytest.fixture(scope="module", params=LINEAR_RUNS, ids=_id)
def setup(request):
    n, dim, h, mode, small = request.param
    c = linear_case(n, dim, h, mode)
    return c, linear_bar(c), small


def test_cases_reach_every_mask_with_every_value():
    """The list itself: every n, dim and out_dim in all three modes, every out_dim with an n that is no multiple of 32, a concat seam
    inside a panel, more than one 128-column block, a wholly empty 64-row tile."""
    for idx, vals in ((0, (1, 31, 32, 33, 63, 64, 65, 129)), (1, (1, 7, 31, 32, 33, 50, 64, 100, 1433)),
                      (2, (1, 3, 31, 32, 33, 50, 96, 97, 127, 128, 129, 300))):
        assert {r[idx] for r in LINEAR_RUNS} == set(vals)
        for v in vals:
            assert {r[3] for r in LINEAR_RUNS if r[idx] == v} == set(LINEAR_MODES), f"{('n', 'dim', 'out_dim')[idx]} = {v}"
    for h in {r[2] for r in LINEAR_RUNS}:
        assert any(r[0] % 32 for r in LINEAR_RUNS if r[2] == h), f"out_dim = {h} only with whole 32-row accumulators"
    assert {r[0] for r in LINEAR_RUNS if r[1] == 1433} == {65}
    assert any(r[3] != "gcn" and r[1] % 32 for r in LINEAR_RUNS)
    assert any(r[2] > 128 for r in LINEAR_RUNS)
    empty = [(r, nd) for r in LINEAR_RUNS for nd in linear_n_devs(r[0], r[4]) if nd is not None and -(-nd // 64) < -(-r[0] // 64)]
    assert empty and any(-(-r[0] // 64) - -(-nd // 64) >= 2 for r, nd in empty)       # ... and one case with two of them
    assert max(r[0] * r[1] * (1 if r[3] == "gcn" else 2) * r[2] for r in LINEAR_RUNS) == 65 * 2866 * 128
    assert len(LINEAR_SHAPES) * 3 == len(LINEAR_RUNS)


def test_generator_is_what_the_bar_assumes(setup):
    """+-U[0.5, 1) everywhere the kernel may look, operands based one float into allocations with odd pads, a self_index without a
    fixed point into a taller table whose spare row is NaN; and a row count leaves NaN exactly where the kernel must not read."""
    c, _, small = setup
    n, dim, h = c["n"], c["dim"], c["out_dim"]
    x, w = linear_operands(c)
    assert x.dtype == np.float32 and w.dtype == np.float32 and x.shape == (n, w.shape[1]) and w.shape[0] == h
    for t in (x, w):
        assert np.all((np.abs(t) >= 0.5) & (np.abs(t) < 1.0))
    for name, width in (("agg", dim), ("self", dim), ("w", 2 * dim), ("out", h)):
        if c[name] is not None:
            off, ld = c[name]
            assert off >= 1 and ld - width in (1, 3, 5), f"{name}: offset {off}, ld {ld} for a width of {width}"
    assert c["w"][0] == 1 + (dim if c["mode"] == "gcn" else 0)    # gcn: the agg half of the concat W
    if c["mode"] == "concat_index":
        idx = c["self_index"]
        assert len(set(idx.tolist())) == n and idx.max() < n + 2 and not np.any(idx == np.arange(n)) and c["tab_rows"] == n + 3
    for nd in linear_n_devs(n, small)[1:]:
        p = linear_poisoned(c, nd)
        xp, _ = linear_operands(p)
        assert np.isnan(xp[nd:]).all() and not np.isnan(xp[:nd]).any()
        assert np.array_equal(xp[:nd], x[:nd])


def test_both_variants_meet_the_bar_and_the_bar_has_teeth(setup):
    c, (bar, figs, share), small = setup
    x, w = linear_operands(c)
    for v in LINEAR_VARIANTS:
        units, _ = contraction_units(linear_act_emulate(c, variant=v), x, w)
        assert units.max() == figs[v] and figs[v] <= bar
        assert figs[v] <= 2.0, f"{v}: {figs[v]:.2f} units: not the plain fp32 accumulation the bar was argued from"
    assert bar < share / 8, f"bar {bar:.2f} against a smallest term of {share:.0f} units"


def test_row_count_mask_of_the_emulation(setup):
    """Rows at or past the row count are neither read nor stored, whatever they hold; the others are the full call's."""
    c, _, small = setup
    full = linear_act_emulate(c)
    for nd in linear_n_devs(c["n"], small)[1:]:
        got = linear_act_emulate(linear_poisoned(c, nd), nn=nd, fill=-31.5)
        assert np.array_equal(got[:nd], full[:nd]) and np.all(got[nd:] == -31.5)


@pytest.mark.parametrize("broken", LINEAR_BROKEN)
def test_broken_arithmetic_misses_the_bar(setup, broken):
    c, (bar, figs, share), small = setup
    if not linear_broken_applies(broken, c):
        return                                                    # this case cannot tell: the faithful emulation, bit for bit
    x, w = linear_operands(c)
    for v in LINEAR_VARIANTS:
        units, _ = contraction_units(linear_act_emulate(c, variant=v, broken=broken), x, w)
        assert units.max() > bar, f"{broken} ({v}): {units.max():.2f} <= bar {bar:.2f}"


@pytest.mark.parametrize("broken", LINEAR_BROKEN)
def test_a_defect_that_does_not_apply_changes_nothing(setup, broken):
    c, _, small = setup
    if linear_broken_applies(broken, c):
        return
    assert np.array_equal(linear_act_emulate(c, broken=broken), linear_act_emulate(c))
