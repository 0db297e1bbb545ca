"""The two-launch ("split") layer 1, kernel by kernel and element by element, against fp64 at its edge shapes: the column-sliced
gather-mean (csrc/sage_gather.hip, csrc/sage_gather_body.h) and the split-bf16 contraction dense_bf16x3_kernel (csrc/sage_dense.hip).

A. ops.gather_mean on row-major tables: the row-per-wave kernel (16-byte and 4-byte loads) and the pipelined sliced kernel with
   16-lane and 32-lane slices, on hand-made lists (util.gather_case), with hash slots on and off, the 0/0 flag 1 and 0, a
   device-side row count below n, and strided table and output views.
B. The same gather on a slice-major table (the rows form) and the contraction, through TwoHopEngine with keep_means on hand-made
   graphs whose degrees are at most the fanouts (util.split_graph: the row order of layer 1 is pinned where it matters): agg1
   against the fp64 mean over the recorded lists, h1 against fp64 [self | agg1 as the device left it] . W1^T, so that the
   contraction is judged alone.
C. The contraction's exact-redo list overflowing its 28 entries, in a child process with 32 persistent blocks.

Bars (tests/util.py; tests/test_split_layer1_host.py shows that faithful fp32 arithmetic meets them and broken arithmetic does not):
gather, derived: |got - ref| <= 1.01 (ceff + 2) 2^-24 sum_j |x_j| / ceff per element; contraction, in units of 2^-23 sum_k |x_k||w_k|
per element: 4 (gcn) / 6 (concat) up to K = 512 and 6 beyond, or twice torch's fp32 mm on the same data, whichever is larger.
Measured on MI355X, per shape class: DESIGN.md section 6.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sage355 import ops
from sage355.engine import TwoHopEngine
from util import (contraction_bar, contraction_units, gather_case, gather_form, gather_miss, gather_reference, split_data,
                  split_graph, split_lists)

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -31.5


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ A. ops.gather_mean
def check_gather(n, k, dim, form, lanes=64, odd_ld=False):
    """One (n, k, dim) through ops.gather_mean: slots on / off x flag 1 / 0, each with n_dev < n into a sentinel-filled strided
    out.  The table is a column slice of a wider array: 16 bytes in with ld = dim + 8, or (odd_ld) 4 bytes in with ld = dim + 5,
    which takes the 16-byte loads away from a width that would have them."""
    ld = dim + (5 if odd_ld else 8)
    ldo = dim + 4
    got_form, got_lanes, trip = gather_form(dim, ld, ldo, n, k, aligned=not odd_ld)
    assert (got_form, got_lanes) == (form, lanes), f"dim={dim} n={n} k={k}: dispatches to {got_form}/{got_lanes}, not {form}/{lanes}"
    c = gather_case(n, k, dim, trip, seed=n + 3 * k + dim)
    T = c["table"].shape[0]
    big = torch.zeros(T, ld)
    off = 1 if odd_ld else 4
    big[:, off:off + dim] = torch.from_numpy(c["table"])
    table = big.to(DEV)[:, off:off + dim]
    assert (table.data_ptr() % 16 == 0) == (not odd_ld)
    n_dev = n - 3 if n > 3 else n - 1
    ndev_t = torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    rs = np.random.default_rng(n + k)
    sperm = rs.permutation(2 * T)
    slot_rows = np.full(2 * T, -1, dtype=np.int32)
    slot_rows[sperm[:T]] = np.arange(T)
    self_slots = np.where(c["self"] >= 0, sperm[np.maximum(c["self"], 0)], np.where(np.arange(n) % 2 == 0, -1, sperm[T + np.arange(n) % T]))
    cnt_t = _i32(c["cnt"])
    for flag in (1, 0):
        ref, bar, ceff = gather_reference(c["table"], c["nbr"], c["cnt"], c["self"], flag)
        flag_t = torch.tensor([flag], dtype=torch.int32, device=DEV)
        for slots in (False, True):
            obig = torch.full((n, ldo), SENTINEL, device=DEV)
            if slots:
                ops.gather_mean(table, _i32(sperm[c["nbr"]]), cnt_t, slot_rows=_i32(slot_rows), self_row=_i32(self_slots),
                                any_nonempty=flag_t, n_dev=ndev_t, out=obig[:, :dim])
            else:
                ops.gather_mean(table, _i32(c["nbr"]), cnt_t, self_row=_i32(c["self"]), any_nonempty=flag_t, n_dev=ndev_t, out=obig[:, :dim])
            torch.cuda.synchronize()
            o = obig.cpu()
            tag = f"{form}/{lanes} dim={dim} n={n} k={k} flag={flag} slots={slots}"
            miss = gather_miss(o[:n_dev, :dim].numpy(), ref[:n_dev], bar[:n_dev], ceff[:n_dev])
            assert miss is None, f"{tag}: {miss}"
            assert torch.equal(o[n_dev:].view(torch.int32), torch.full_like(o[n_dev:], SENTINEL).view(torch.int32)), \
                f"{tag}: a row at or past n_dev = {n_dev} was written"
            assert bool((o[:, dim:] == SENTINEL).all()), f"{tag}: a column at or beyond dim of the strided out was written"


WAVE_KS = (1, 7, 8, 9, 64, 65, 100)
WAVE = [(4, False, WAVE_KS), (252, False, WAVE_KS), (260, False, (65, 100)),          # 16-byte loads (260 with k <= 64 is a sliced shape)
        (50, False, WAVE_KS), (1433, False, WAVE_KS),                                  # 4-byte loads by width
        (252, True, WAVE_KS), (260, True, WAVE_KS)]                                    # ... and by an odd ld


@pytest.mark.parametrize("dim,odd_ld,ks", WAVE, ids=lambda v: str(v) if not isinstance(v, tuple) else "k" + "_".join(map(str, v)))
def test_gather_row_per_wave(dim, odd_ld, ks):
    """gather_mean_kernel<4> / <1> at n = 65: one and two 256-column blocks (252 / 260), the 8-loads-in-flight tail, a second page
    of 64 ids (65, 100)."""
    form = "wave1" if (odd_ld or dim % 4) else "wave4"
    for k in ks:
        check_gather(65, k, dim, form, odd_ld=odd_ld)


SLICED16_KS = (1, 8, 9, 16, 17, 32, 33, 64)          # U = 2 (k <= 8), 4 (<= 16), 8 and, past 32, its second trip


@pytest.mark.parametrize("n", [1, 5, 67])
@pytest.mark.parametrize("dim", [260, 320, 500])
def test_gather_sliced_16_lanes_wide_rows(dim, n):
    """Rows wider than 256 floats are sliced at any n: a last slice one lane wide (260), whole (320), partial (500)."""
    for k in SLICED16_KS:
        check_gather(n, k, dim, "sliced", 16)


@pytest.mark.parametrize("k", SLICED16_KS)
@pytest.mark.parametrize("dim", [64, 128, 192, 256])
def test_gather_sliced_16_lanes_large_layers(dim, k):
    check_gather(8192 + 3, k, dim, "sliced", 16)


@pytest.mark.parametrize("k", [8, 9, 16, 17, 64])     # U = 4 (k <= 8), 8 and, past 16, further trips
@pytest.mark.parametrize("dim", [68, 100, 124])
def test_gather_sliced_32_lanes(dim, k):
    """Narrow rows that do not end on a 64-float boundary are ONE 32-lane slice (two neighbours per wave-instruction)."""
    check_gather(8192 + 3, k, dim, "sliced", 32)


# ----------------------------------------------------------------------------------------- B. gather + contraction in the engine
def run_engine_case(d0, h1, rows, k1, concat, self_loop, prepare, slice_major):
    """-> the contraction's figure of one case (and asserts).  split_graph gives `rows` layer-1 rows; the forward gets seeds[:b]
    of a larger max_batch, so the kernels read the row count on the device."""
    g = split_graph(rows, k1, concat, self_loop, seed=d0 + rows)
    N, b, k2 = g["num_nodes"], g["b"], 64
    max_batch = max(b + 3, 128) if d0 <= 256 else b + 3
    tab, w = split_data(g, d0, h1, concat, seed=d0 + h1 + rows)
    unaligned = d0 in (100, 500)                       # a table view the 16-byte kernels cannot take: the engine's padded private copy
    tbig = torch.zeros(N, d0 + 3 if unaligned else d0)
    (tbig[:, 1:1 + d0] if unaligned else tbig).copy_(torch.from_numpy(tab))
    tbig = tbig.to(DEV)
    table = tbig[:, 1:1 + d0] if unaligned else tbig
    m = 2 if concat else 1
    w2 = torch.zeros(8, m * h1, device=DEV)
    pad = np.zeros(1, dtype=np.int32)                  # (a CSR without edges still needs an address)
    eng = TwoHopEngine(torch.from_numpy(g["rowptr_in"]).to(DEV), _i32(np.concatenate([g["col_in"], pad])), table, torch.from_numpy(w).to(DEV),
                       w2, k1, k2, concat=concat, agg_self_loop=self_loop, act1=ops.ACT_NONE, act2=ops.ACT_NONE, nan_empty=True,
                       max_batch=max_batch, rowptr_outer=torch.from_numpy(g["rowptr_out"]).to(DEV),
                       col_outer=_i32(np.concatenate([g["col_out"], pad])), prepare_weights=prepare,
                       slice_major="auto" if slice_major is None else slice_major)
    eng.keep_means = True
    tag = f"d0={d0} h1={h1} rows={rows} k1={k1} concat={concat} self_loop={self_loop} prepare={prepare} slice_major={slice_major}"
    assert bool(eng.layout.layer1_split), f"{tag}: layer 1 is not split"
    assert eng.layout.max_s1 > rows and (d0 > 256 or eng.layout.max_s1 >= 8192)
    seeds = torch.arange(max_batch, dtype=torch.int32, device=DEV)
    eng.forward(seeds[:b], seed=5)
    it = eng.intermediates()
    s1 = it["s1_nodes"].cpu().numpy().astype(np.int64)
    nbr1, cnt1 = it["nbr1"].cpu().numpy().astype(np.int64), it["cnt1"].cpu().numpy().astype(np.int64)
    # a case must not pass on another kernel
    assert it["agg1"] is not None, f"{tag}: the means were not kept"
    assert (eng._table_sliced is not None) == bool(slice_major), f"{tag}: slice-major copy {'missing' if slice_major else 'present'}"
    assert (eng._model(keep_means=True).w1_prepared is not None) == prepare
    assert (eng.table is not table) == unaligned
    assert it["n_s1"] == rows and (not concat or np.array_equal(s1[:b], np.arange(b)))
    assert sorted(s1.tolist()) == sorted(g["order"].tolist())
    # ... nor on rows that are not where the edges are: the last row ends a chunk, the row before it takes the exact path
    assert int(s1[-1]) in g["ender"] and (g["mate"][int(s1[-1])] < 0 or s1[-2] == g["mate"][int(s1[-1])]), f"{tag}: row order {s1[-3:]}"
    want_nbr, want_cnt = split_lists(g, s1, k1)
    assert np.array_equal(cnt1, want_cnt), f"{tag}: the sampler did not take whole neighbourhoods"
    live = np.arange(k1)[None, :] < cnt1[:, None]
    assert np.array_equal(np.sort(np.where(live, nbr1, -1), 1), np.sort(np.where(live, want_nbr, -1), 1))
    # the gather, alone
    agg_dev = it["agg1"].cpu().numpy()
    ref, bar, ceff = gather_reference(tab, nbr1, cnt1, s1 if self_loop else None, 1)
    miss = gather_miss(agg_dev, ref, bar, ceff)
    assert miss is None, f"{tag}: agg1: {miss}"
    nanrow = np.isnan(agg_dev).any(1)
    assert nanrow.sum() == (1 if (g["iso"] >= 0 and not self_loop) else 0)
    assert not nanrow.any() or (s1[nanrow][0] == g["iso"] and 0 < np.nonzero(nanrow)[0][0] % 32 < 31)      # in the middle of a tile
    # the contraction, alone: fp64 on the device's own fp32 means
    x = np.concatenate([tab[s1], agg_dev], 1) if concat else agg_dev
    h1_dev = it["h1"].cpu().numpy()
    assert np.array_equal(np.isnan(h1_dev), np.repeat(nanrow[:, None], h1, 1)), f"{tag}: h1's NaN rows are not agg1's"
    units, _ = contraction_units(np.nan_to_num(h1_dev), x, w)
    limit, e_torch = contraction_bar(x, w, concat)
    huge_rows = np.nonzero((np.abs(np.nan_to_num(x)) >= 2.0 ** 127).any(1))[0]
    assert sorted(s1[huge_rows].tolist()) == sorted(g["huge"]), f"{tag}: the exact-path rows are {s1[huge_rows]}"
    worst = float(units.max())
    r, c = np.unravel_index(np.argmax(units), units.shape)
    print(f"SPLIT1 {tag} K={m * d0}: contraction {worst:.2f} x 2^-23 sum|x||w| at row {r} column {c} (bar {limit:.2f}, torch fp32 mm "
          f"{e_torch:.2f}; exact-path rows {huge_rows.tolist()[-3:]}, NaN row {np.nonzero(nanrow)[0].tolist()})")
    assert worst <= limit, (f"{tag}: h1[{r}, {c}] is {worst:.2f} x 2^-23 sum|x||w| from fp64, bar {limit:.2f} "
                            f"(torch fp32 mm on the same data: {e_torch:.2f})")
    return worst


# (d0, h1, layer-1 rows, k1, concat, self-loop aggregator, prepare_weights, slice_major (None: the shape has no slice-major copy)).
# Kernel instantiations: KP 64 (d0 = 64), KP 128 (68, 100, 128), KP 256 (132, 252, 256), MP (260 .. 516), each gcn / concat and with
# W1 as prepared planes / as it is.  Every h1 and every row count meets every KP / MP class, both encoders and both W1 forms.
ENGINE_CASES = [
    (64, 1, 1, 1, False, False, False, False),
    (64, 4, 31, 15, True, False, False, True),
    (64, 32, 32, 16, False, True, True, False),
    (64, 36, 33, 17, True, False, True, True),
    (64, 50, 127, 33, False, False, False, False),
    (64, 100, 128, 64, True, False, True, True),
    (64, 124, 129, 8, False, True, True, False),
    (64, 128, 1, 9, True, False, True, True),
    (100, 1, 32, 17, True, False, True, None),
    (128, 4, 33, 33, False, False, True, True),
    (68, 32, 127, 64, True, False, False, None),
    (100, 36, 128, 8, False, False, False, None),
    (128, 50, 129, 9, True, False, True, False),
    (68, 100, 1, 1, False, False, True, None),
    (100, 124, 31, 15, True, False, False, None),
    (128, 128, 32, 16, False, False, False, True),
    (256, 1, 127, 8, False, False, False, True),
    (132, 4, 128, 9, True, False, False, None),
    (252, 32, 129, 1, False, True, True, None),
    (256, 36, 1, 15, True, False, True, False),
    (132, 50, 31, 16, False, False, False, None),
    (252, 100, 32, 17, True, False, False, None),
    (256, 124, 33, 33, False, True, True, True),
    (132, 128, 127, 64, True, False, True, None),
    (512, 1, 129, 15, True, False, True, True),
    (516, 4, 1, 16, False, False, True, None),
    (260, 32, 31, 17, True, False, False, None),
    (320, 36, 32, 33, False, False, False, False),
    (500, 50, 33, 64, True, False, True, None),
    (512, 100, 127, 8, False, False, True, False),
    (516, 124, 128, 9, True, False, False, None),
    (260, 128, 129, 1, False, False, False, None),
    # the rows form (slice-major table: 8-lane slices, TRIP 16) at k1 = 1, 15, 16, 17, 33, 64 with row counts that are no multiple
    # of 8, and the row-major kernels at the same widths
    (64, 128, 33, 1, False, False, True, True),
    (128, 32, 127, 15, False, False, False, True),
    (256, 128, 129, 16, False, True, True, True),
    (320, 36, 31, 17, False, False, True, True),
    (512, 124, 33, 33, False, False, False, True),
    (256, 100, 127, 64, True, False, True, True),
    (128, 4, 129, 64, True, False, False, True),
    (64, 50, 31, 17, True, False, True, True),
    (512, 1, 1, 16, True, False, True, True),
    (256, 128, 33, 15, False, False, False, False),
    (512, 32, 129, 33, False, False, True, False),
    (64, 124, 127, 64, False, True, False, False),
    # more than one tile per persistent block (rows > 32 x 224), and a second group of four tiles per block of the two-pass concat
    # kernel (rows > 4 x 32 x 224)
    (128, 128, 32 * 224 + 37, 15, False, False, True, True),
    (256, 128, 4 * 32 * 224 + 5, 9, True, False, True, None),
    (256, 36, 32 * 224 + 33, 8, False, False, False, False),
    (516, 128, 32 * 224 + 1, 7, True, False, False, None),
]


def _engine_id(c):
    d0, h1, rows, k1, concat, self_loop, prepare, sm = c
    return (f"d{d0}-h{h1}-r{rows}-k{k1}-{'concat' if concat else 'gcn'}{'-selfloop' if self_loop else ''}-"
            f"{'prep' if prepare else 'raw'}-{'rowmajor' if not sm else 'slicemajor'}")


@pytest.mark.parametrize("case", ENGINE_CASES, ids=_engine_id)
def test_engine_split_layer1_gather_and_contraction(case):
    run_engine_case(*case)


def test_engine_cases_reach_every_instantiation_with_every_value():
    """The parametrisation above, checked: every d0 / h1 / row count the kernels' masks distinguish, each h1 and row count with
    every K class, encoder and W1 form, all 16 (K class, CONCAT, PREP) instantiations, and the rows form at every k1."""
    cls = lambda d0: 64 if d0 <= 64 else 128 if d0 <= 128 else 256 if d0 <= 256 else 0
    assert {c[0] for c in ENGINE_CASES} == {64, 68, 100, 128, 132, 252, 256, 260, 320, 500, 512, 516}
    for idx, vals in ((1, (1, 4, 32, 36, 50, 100, 124, 128)), (2, (1, 31, 32, 33, 127, 128, 129))):
        for v in vals:
            mine = [c for c in ENGINE_CASES if c[idx] == v]
            assert {cls(c[0]) for c in mine} == {64, 128, 256, 0} and {c[4] for c in mine} == {False, True} and {c[6] for c in mine} == {False, True}
    assert len({(cls(c[0]), c[4], c[6]) for c in ENGINE_CASES}) == 16
    sliced = [c for c in ENGINE_CASES if c[7]]
    assert {1, 15, 16, 17, 33, 64} <= {c[3] for c in sliced} and any(c[2] % 8 for c in sliced)
    assert {c[0] for c in ENGINE_CASES if c[7] is False} == {c[0] for c in sliced} == {64, 128, 256, 320, 512}
    assert any(c[5] for c in ENGINE_CASES) and any(c[2] > 32 * 224 for c in ENGINE_CASES)
    assert any(c[4] and c[0] == 256 and c[2] > 4 * 32 * 224 for c in ENGINE_CASES)


# ------------------------------------------------------------------------------------------ C. the exact-redo list overflows
def redo_list_overflow_check():
    """d0 = 64, h1 = 4, concat, 32 x 32 x 29 + 5 layer-1 rows on 32 persistent blocks: every block owns 29 or 30 tiles and every
    tile holds a row with a 3e38 entry (rows [0, b) are the seeds in order: the row of tile t is 32 t + t % 32; the last tile is
    the five frontier nodes, all marked), so every block's list passes its 28 entries and the block redoes all its tiles' marked
    rows.  Inf / NaN classes as torch's fp32 mm, values against fp64."""
    assert os.environ.get("SAGE_DENSE_BLOCKS") == "32"
    d0, h1, rows, f = 64, 4, 32 * 32 * 29 + 5, 5
    b = rows - f
    nl = b + f                                                   # seeds [0, b), frontier [b, nl): seed i < 5 -> frontier node b + i
    N = 2 * nl                                                   # node v's one inner neighbour: nl + v; seed 13 has none (a 0/0 row)
    deg = (np.arange(N) < nl).astype(np.int64)
    deg[13] = 0
    rowptr_in = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col_in = (nl + np.nonzero(deg)[0]).astype(np.int32)
    rowptr_out = np.concatenate([[0], np.cumsum(np.arange(N) < f)]).astype(np.int64)
    col_out = (b + np.arange(f)).astype(np.int32)
    rs = np.random.default_rng(7)
    tab = rs.standard_normal((N, d0)).astype(np.float32)
    w = (rs.standard_normal((h1, 2 * d0)) / 12).astype(np.float32)
    t = np.arange(b // 32)
    tab[32 * t + t % 32, 1 + t % 7] = 3.0e38
    tab[b:b + f, 3] = -3.0e38
    eng = TwoHopEngine(torch.from_numpy(rowptr_in).to(DEV), _i32(col_in), torch.from_numpy(tab).to(DEV), torch.from_numpy(w).to(DEV),
                       torch.zeros(8, 2 * h1, device=DEV), 1, 1, concat=True, act1=ops.ACT_NONE, act2=ops.ACT_NONE, nan_empty=True,
                       max_batch=b + 3, rowptr_outer=torch.from_numpy(rowptr_out).to(DEV), col_outer=_i32(col_out))
    eng.keep_means = True
    assert bool(eng.layout.layer1_split)
    eng.forward(torch.arange(b + 3, dtype=torch.int32, device=DEV)[:b], seed=3)
    it = eng.intermediates()
    assert it["n_s1"] == rows and it["agg1"] is not None
    s1 = it["s1_nodes"].cpu().numpy().astype(np.int64)
    x = np.concatenate([tab[s1], it["agg1"].cpu().numpy()], 1)
    marked = (np.abs(np.nan_to_num(x)) >= 2.0 ** 127).any(1) | np.isnan(x).any(1)
    per_tile = np.add.reduceat(marked, np.arange(0, rows, 32))
    assert (per_tile >= 1).all() and len(per_tile) == 929 and (per_tile < 32).all()
    assert min(np.bincount(np.arange(929) % 32)) > 28           # tiles per block > the list's capacity
    got = it["h1"].cpu()
    ref32 = torch.from_numpy(x) @ torch.from_numpy(w).t()
    assert torch.equal(torch.isnan(got), torch.isnan(ref32))
    assert torch.equal(torch.isposinf(got), torch.isposinf(ref32)) and torch.equal(torch.isneginf(got), torch.isneginf(ref32))
    assert int(torch.isnan(got).any(1).sum()) == 1               # the isolated seed's 0/0 row
    units, _ = contraction_units(np.nan_to_num(got.numpy()), x, w)
    limit, e_torch = contraction_bar(x, w, True)
    print(f"SPLIT1 redo-list overflow: contraction {units.max():.2f} x 2^-23 sum|x||w| (bar {limit:.2f}, torch fp32 mm {e_torch:.2f})")
    assert units.max() <= limit, f"{units.max():.2f} x 2^-23 sum|x||w| (torch fp32 mm: {e_torch:.2f})"


OVERFLOW_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {repo!r} + "/graphsage-simple_amd", {repo!r} + "/tests"]
import test_gpu_split_layer1 as t
t.redo_list_overflow_check()
print("OVERFLOW_OK")
"""


def test_contraction_redo_list_overflow_in_a_child_process(tmp_path):
    """SAGE_DENSE_BLOCKS is read once per process: a fresh child, under its own timeout."""
    script = tmp_path / "overflow.py"
    script.write_text(OVERFLOW_CHILD.format(repo=REPO))
    e = dict(os.environ)
    e["SAGE_DENSE_BLOCKS"] = "32"
    res = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, timeout=300)
    print(res.stdout[-600:])
    assert res.returncode == 0 and "OVERFLOW_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
