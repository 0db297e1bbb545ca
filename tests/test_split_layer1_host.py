"""The bars of tests/test_gpu_split_layer1.py have teeth and are reachable: numpy fp32 emulations of the split layer 1's arithmetic
on the very data generators of that module (tests/util.py).

Gather: both summation orders of csrc/sage_gather_body.h -- lane-group partial sums met by an xor tree (the column-sliced kernels:
group g of 64 / lanes sums the neighbours j = g mod groups in list order, group 0 adds the self row, then the tree) and plain list
order (the rows form and the row-per-wave kernel) -- times the rounded reciprocal of the set size.  Contraction: the three-term bf16
split of csrc/sage_split_bf16.h (round to nearest even, exact remainders), the six products of mfma_bf16x3_step smallest first, one
fp32 rounding per 16-column matrix instruction, the two K halves of a pass accumulated apart and added last, passes as
dense_bf16x3_kernel walks them (both chunks in one pass below 256 columns, one chunk per pass at 256, 256-column passes above).

The faithful emulations meet the bars; each broken one misses its bar at every shape class.
"""
import numpy as np
import pytest

from util import (contraction_bar, contraction_units, gather_case, gather_miss, gather_reference, split_data, split_graph,
                  split_lists)

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ the gather
def emulate_gather(table, nbr, cnt, self_eff, flag, lanes=None, broken=None):
    """fp32 mean as the kernels sum it.  lanes = 8 / 16 / 32: partial sums of 64 / lanes lane groups and the xor tree; None: list
    order.  broken: "div_c" divides by the list length instead of the set size, "skip_last" leaves out the last valid neighbour,
    "self_pos0" looks for the self row at list position 0 only."""
    n, k = nbr.shape
    dim = table.shape[1]
    groups = 1 if lanes is None else 64 // lanes
    acc = np.zeros((groups, n, dim), dtype=F32)
    used = cnt - 1 if broken == "skip_last" else cnt
    inlist = np.zeros(n, dtype=bool)
    for j in range(k):
        m = j < used
        acc[j % groups] += np.where(m[:, None], table[nbr[:, j]], F32(0))
        if self_eff is not None and (broken != "self_pos0" or j == 0):
            inlist |= (j < cnt) & (nbr[:, j] == self_eff)
    extra = np.zeros(n, dtype=bool) if self_eff is None else (self_eff >= 0) & ~inlist
    if extra.any():
        acc[0] += np.where(extra[:, None], table[np.maximum(self_eff, 0)], F32(0))
    step = 1
    while step < groups:                                          # acc[g] += acc[g ^ step], all groups at once
        acc = acc + acc[np.arange(groups) ^ step]
        step *= 2
    ceff = cnt + extra
    div = cnt if broken == "div_c" else ceff
    with np.errstate(divide="ignore", invalid="ignore"):
        res = acc[0] * (F32(1) / div.astype(F32))[:, None]
    res[ceff == 0] = np.nan if flag else 0.0
    return res


# (n, k, dim, lanes, ids per trip): the row-per-wave kernel (list order, 8 loads in flight) with 16-byte and 4-byte loads, the
# 16-lane and 32-lane sliced kernels at their U = 2 / 4 / 8 selections and second trips, the rows form (8-lane slices, TRIP 16)
GATHER_SHAPES = [
    (65, 7, 4, None, 8), (65, 100, 252, None, 8), (65, 65, 260, None, 8), (65, 9, 50, None, 8), (65, 64, 1433, None, 8),
    (67, 8, 260, 16, 8), (5, 17, 500, 16, 32), (67, 33, 320, 16, 32), (8195, 16, 128, 16, 16), (8195, 64, 256, 16, 32),
    (8195, 9, 68, 32, 16), (8195, 64, 124, 32, 16), (8195, 8, 100, 32, 8),
    (129, 17, 64, 8, 16), (33, 64, 512, 8, 16), (127, 15, 320, 8, 16),
]


@pytest.fixture(scope="module", params=GATHER_SHAPES, ids=lambda s: "n{}-k{}-d{}-l{}-t{}".format(*s))
def gather_setup(request):
    n, k, dim, lanes, trip = request.param
    c = gather_case(n, k, dim, trip, seed=n + 3 * k + dim)
    return c, lanes, {flag: gather_reference(c["table"], c["nbr"], c["cnt"], c["self"], flag) for flag in (1, 0)}


def test_gather_generator_holds_every_edge(gather_setup):
    """What the issue asks of the inputs, asserted on the generator itself: list lengths 0, 1, k - 1, k and around every trip
    boundary; self rows absent, at position 0, at the last valid position, in every later trip and (k > 64) at positions >= 64."""
    c, _, refs = gather_setup
    n, k = c["nbr"].shape
    cnt, mode, pos, trip = c["cnt"], c["mode"], c["pos"], c["trip"]
    if n >= 65:
        want = {k, 0, 1, k - 1} | {b + d for b in range(trip, k + 1, trip) for d in (-1, 0, 1)}
        assert {v for v in want if 0 <= v <= k} <= set(cnt.tolist())
        assert set(mode.tolist()) == set(range(6))
        later = (mode == 4) & (cnt > trip)
        if k > trip:
            assert later.any() and (pos[later] >= trip).all()
        if n >= 6 * 64:
            assert {int(p) // trip for p in pos[later]} == set(range(1, (k - 1) // trip + 1)) or k <= trip
        if k > 64:
            assert ((mode == 5) & (pos >= 64)).any()
    if n >= 2:
        assert (refs[1][2] == 0).any()                            # an empty set
    assert all(len(set(r[:c_])) == c_ for r, c_ in zip(c["nbr"][:200], cnt[:200]))
    heavy = np.abs(c["table"]).max(1)
    rows = np.nonzero(cnt > 0)[0][:200]
    assert all(heavy[c["nbr"][r, cnt[r] - 1]] >= heavy[c["nbr"][r, :cnt[r]]].max() for r in rows if cnt[r] > 1)
    if c["table"].shape[1] > 4:
        assert (np.abs(c["table"][:, -4:]).min(1) >= np.abs(c["table"][:, :-4]).max(1)).all()      # inside every row


@pytest.mark.parametrize("flag", [1, 0])
def test_faithful_gather_orders_meet_the_bar(gather_setup, flag):
    c, lanes, refs = gather_setup
    ref, bar, ceff = refs[flag]
    for order in {lanes, None}:
        got = emulate_gather(c["table"], c["nbr"], c["cnt"], c["self"], flag, lanes=order)
        assert gather_miss(got, ref, bar, ceff) is None, f"lanes={order}: {gather_miss(got, ref, bar, ceff)}"


@pytest.mark.parametrize("broken", ["div_c", "skip_last", "self_pos0"])
def test_broken_gathers_miss_the_bar(gather_setup, broken):
    c, lanes, refs = gather_setup
    ref, bar, ceff = refs[1]
    got = emulate_gather(c["table"], c["nbr"], c["cnt"], c["self"], 1, lanes=lanes, broken=broken)
    assert gather_miss(got, ref, bar, ceff) is not None


# ------------------------------------------------------------------------------------------------------------- the contraction
def bf16_round(x):
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    u = (u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def split3(x):
    hi = bf16_round(x)
    r1 = (x - hi).astype(F32)
    mid = bf16_round(r1)
    lo = bf16_round((r1 - mid).astype(F32))
    return hi, mid, lo


def emulate_contraction(x, w, d0, concat, broken=None):
    """[self | agg] . W^T as dense_bf16x3_kernel forms it (see the module docstring).  broken: "drop_low" leaves the two products
    with a low bf16 term out of the 16-column step that holds the last K column, "zero_last4" zeroes the last four K columns of
    the rows, "omit_last_out" never writes the last output column."""
    x = np.array(x, dtype=F32)
    n, h = x.shape[0], w.shape[0]
    chunks = 2 if concat else 1
    kp = 64 if d0 <= 64 else 128 if d0 <= 128 else 256
    mp = d0 > 256
    if broken == "zero_last4":
        x[:, -4:] = 0
    passes = []                                                   # per pass: the (chunk, column) of every K slot, -1 = masked
    if mp:
        for ch in range(chunks):
            for p in range(-(-d0 // 256)):
                col = p * 256 + np.arange(256)
                passes.append(np.where(col < d0, ch * d0 + col, -1))
    else:
        pch = 2 if (concat and kp < 256) else 1
        for p in range(chunks // pch):
            kk = np.arange(pch * kp)
            col = kk % kp
            passes.append(np.where(col < d0, (p * pch + kk // kp) * d0 + col, -1))
    acc = [np.zeros((n, h), dtype=F32), np.zeros((n, h), dtype=F32)]
    last_k = chunks * d0 - 1
    for idx in passes:
        a = np.where(idx >= 0, x[:, np.maximum(idx, 0)], F32(0)).astype(F32)
        b = np.where(idx >= 0, w[:, np.maximum(idx, 0)], F32(0)).astype(F32)
        ah, am, al = (t.astype(np.float64) for t in split3(a))
        bh, bm, bl = (t.astype(np.float64) for t in split3(b))
        kh = len(idx) // 2
        for g in range(2):
            for st in range(kh // 16):
                s = slice(g * kh + 16 * st, g * kh + 16 * st + 16)
                prods = [(al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh)]
                if broken == "drop_low" and last_k in idx[s]:
                    prods = prods[2:]
                for pa, pb in prods:
                    acc[g] = (acc[g].astype(np.float64) + pa[:, s] @ pb[:, s].T).astype(F32)
    out = acc[0] + acc[1]
    if broken == "omit_last_out":
        out[:, -1] = 0
    return out


# (d0, h1, layer-1 rows, k1, concat, self-loop aggregator): KP 64 / 128 / 256 and the multi-pass kernel, gcn and concat
CONTRACT_SHAPES = [
    (64, 4, 33, 9, False, False), (64, 36, 31, 16, True, False), (68, 1, 32, 17, False, True), (100, 50, 129, 8, True, False),
    (128, 128, 127, 33, False, False), (132, 100, 33, 15, True, False), (252, 124, 31, 7, False, False), (256, 32, 128, 64, True, False),
    (256, 128, 129, 16, False, True), (260, 4, 33, 9, False, False), (320, 36, 127, 17, True, False), (500, 50, 32, 15, False, False),
    (512, 128, 31, 33, True, False), (516, 100, 129, 8, False, False), (516, 124, 33, 16, True, False),
]


@pytest.fixture(scope="module", params=CONTRACT_SHAPES, ids=lambda s: "d{}-h{}-r{}-k{}-{}{}".format(*s[:4], "concat" if s[4] else "gcn", "-selfloop" if s[5] else ""))
def contract_setup(request):
    d0, h1, rows, k1, concat, self_loop = request.param
    g = split_graph(rows, k1, concat, self_loop, seed=d0 + rows)
    s1 = g["order"]
    nbr1, cnt1 = split_lists(g, s1, k1)
    table, w1 = split_data(g, d0, h1, concat, seed=d0 + h1 + rows)
    table[table == np.float32(3.0e38)] = 1.0                      # (the exact-path rows are the GPU module's business)
    agg = emulate_gather(table, nbr1, cnt1, s1 if self_loop else None, 1, lanes=None)
    x = np.concatenate([table[s1], agg], 1) if concat else agg
    bar, e_torch = contraction_bar(x, w1, concat)
    return d0, concat, x, w1, bar, self_loop, s1


def test_contraction_generator_puts_the_weight_on_the_edges(contract_setup):
    d0, concat, x, w1, bar, self_loop, s1 = contract_setup
    fin = ~np.isnan(x).any(1)
    assert (~fin).sum() == (0 if self_loop or len(s1) < 3 else 1)    # the isolated node's 0/0 row (its own row under the self loop)
    prod = np.abs(x[fin])[:, None, :] * np.abs(w1)[None, :, :]    # [rows, h1, K]
    for c in range(2 if concat else 1):
        chunk = prod[:, :, c * d0:(c + 1) * d0].mean((0, 1))
        assert chunk[-4:].mean() > 50 * chunk[:-4].mean() and chunk[-4:].min() > 4 * chunk[:-4].mean()     # the last four K columns of every chunk carry the largest products
    assert w1.shape[0] == 1 or np.abs(w1[-1]).mean() > 3 * np.abs(w1[:-1]).mean()
    assert len(s1) == 1 or (fin[-1] and np.abs(x[-1]).sum() > 2 * np.median(np.abs(x[fin]).sum(1)))   # ... and the last row


def test_faithful_contraction_meets_the_bar(contract_setup):
    d0, concat, x, w1, bar, self_loop, s1 = contract_setup
    got = emulate_contraction(np.nan_to_num(x), w1, d0, concat)
    units, ref = contraction_units(got, x, w1)
    assert units.max() <= bar, f"{units.max():.2f} > {bar:.2f}"


@pytest.mark.parametrize("broken", ["drop_low", "zero_last4", "omit_last_out"])
def test_broken_contractions_miss_the_bar(contract_setup, broken):
    d0, concat, x, w1, bar, self_loop, s1 = contract_setup
    got = emulate_contraction(np.nan_to_num(x), w1, d0, concat, broken=broken)
    units, ref = contraction_units(got, x, w1)
    assert units.max() > bar, f"{broken}: {units.max():.2f} <= {bar:.2f}"
