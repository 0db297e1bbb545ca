"""The pair form of the phase-sliced layer 1 (csrc/sage_layer1_phase.hip, layer1_pair_kernel: a block owns two 32-row tiles and walks
them half a phase apart), through ops.layer1_fused, at the shapes where two tiles per block can go wrong.

Bit for bit against the split form.  The split form (sliced gather on the slice-major table, then the dense contraction) is what a
TwoHopEngine with keep_means runs; on a hand-made graph whose degrees are at most the fanouts (util.split_graph) its sampler takes
whole neighbourhoods, so one forward per (d0, h1, k) leaves a POOL of layer-1 rows with their lists and the split form's h1.  A row's
bits depend neither on where it sits nor on how many rows there are, so the one-launch layer 1 on ANY selection of pool rows must
return exactly the pool's h1 of those rows.  The pool holds a row without neighbours (NaN under the 0/0 flag), rows whose list is one
3e38 entry (the exact fp32 path), lists of every length up to k, and -- under the self-loop aggregator -- self rows that are among
their neighbours.

Against fp64: oracle.ref_sparse.gather_mean then linear_act on the same lists, |got - want| <= 1e-5 max|pre-activation row|, NaN
patterns equal (the rule of tests/test_gpu_layer1_fused.py).  Inf entries: torch.mm's classes on the fp32 means, as that file's
special-values test states them; and the rows of the OTHER tile of the pair keep the bits they have without the Inf (the flag is per
tile).

A pair is 64 rows and pairs are dealt to 8 classes, so the row counts sit around 32, 64 and 8 * 64; 2 * CUs * 64 + 33 rows pass the
grid cap of two blocks per CU, so that a block walks a second pair.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_sparse
from sage355 import ops
from sage355.engine import TwoHopEngine
from util import split_data, split_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-5
SENTINEL = -31.5
POOL_ROWS = 129


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _pool(d0, h1, k, self_loop=False, act=ops.ACT_NONE):
    """One split-form forward on split_graph -> the pool: table, w, lists, self rows, h1 of the split form (all on the host) and the
    slice-major table on the device."""
    for seed in range(d0 + k, d0 + k + 64):              # (split_graph deals the list lengths in a cycle that may miss some)
        g = split_graph(POOL_ROWS, k, False, self_loop, seed=seed)
        if {1, k} <= set(g["deg"][:g["nl"]].tolist()):
            break
    N, b = g["num_nodes"], g["b"]
    tab, w = split_data(g, d0, h1, False, seed=d0 + h1 + k)
    table = torch.from_numpy(tab).to(DEV)
    pad = np.zeros(1, dtype=np.int32)
    eng = TwoHopEngine(torch.from_numpy(g["rowptr_in"]).to(DEV), _i32(np.concatenate([g["col_in"], pad])), table,
                       torch.from_numpy(w).to(DEV), torch.zeros(8, h1, device=DEV), k, 64, agg_self_loop=self_loop, act1=act,
                       act2=ops.ACT_NONE, nan_empty=True, max_batch=max(b + 3, 128),
                       rowptr_outer=torch.from_numpy(g["rowptr_out"]).to(DEV), col_outer=_i32(np.concatenate([g["col_out"], pad])),
                       prepare_weights=True, slice_major=True)
    eng.keep_means = True
    assert bool(eng.layout.layer1_split)
    eng.forward(torch.arange(max(b + 3, 128), dtype=torch.int32, device=DEV)[:b], seed=5)
    it = eng.intermediates()
    assert it["agg1"] is not None and eng._table_sliced is not None, "the pool was not made by the split form on the slice-major table"
    n = int(it["n_s1"])
    assert n == POOL_ROWS
    cnt = it["cnt1"].cpu().numpy()[:n].astype(np.int32)
    nbr = it["nbr1"].cpu().numpy()[:n].astype(np.int32)
    nbr[np.arange(k)[None, :] >= cnt[:, None]] = -1
    s1 = it["s1_nodes"].cpu().numpy()[:n].astype(np.int32)
    assert (cnt == k).any() and (cnt == 1).any() and (self_loop or (cnt == 0).any())
    return dict(table=torch.from_numpy(tab), w=torch.from_numpy(w), nbr=nbr, cnt=cnt, self=s1 if self_loop else None,
                h1=it["h1"][:n].cpu().clone(), sliced=ops.slice_major(table), act=act, k=k, d0=d0, h1_dim=h1)


def _fused(p, idx, extra=40, flag=1, table_sliced=None, w=None):
    """ops.layer1_fused on pool rows `idx` as the first len(idx) of len(idx) + extra rows (device-side count) -> those rows; asserts
    that the rest was not written."""
    idx = np.asarray(idx)
    n, cap, k = len(idx), len(idx) + extra, p["k"]
    fill = idx[np.arange(extra) % max(n, 1)] if n else np.zeros(extra, dtype=np.int64)       # live-looking lists past the count
    rows = np.concatenate([idx, fill]).astype(np.int64)
    sr = None if p["self"] is None else _i32(p["self"][rows])
    w = p["w"] if w is None else w
    out = torch.full((cap, w.shape[0] + 4), SENTINEL, device=DEV)[:, :w.shape[0]]
    ops.layer1_fused(p["sliced"] if table_sliced is None else table_sliced, _i32(p["nbr"][rows]), _i32(p["cnt"][rows]), w.to(DEV),
                     act=p["act"], self_row=sr, any_nonempty=None if flag is None else torch.tensor([flag], dtype=torch.int32, device=DEV),
                     n_dev=torch.tensor([n], dtype=torch.int32, device=DEV), out=out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[n:] == SENTINEL).all(), "rows at or past the device-side count were written"
    return got[:n]


ACT_NAME = {ops.ACT_NONE: "none", ops.ACT_RELU: "relu", ops.ACT_SIGMOID: "sigmoid"}


def _assert_fp64(p, idx, got, what):
    idx = np.asarray(idx)
    nbr, cnt = p["nbr"][idx], p["cnt"][idx]
    self_row = None if p["self"] is None else p["self"][idx]
    agg = ref_sparse.gather_mean(p["table"].double(), nbr, cnt, self_idx=self_row, nan_empty=True)
    if self_row is None:
        agg[torch.from_numpy(cnt == 0)] = float("nan")
    pre = agg.mm(p["w"].double().t())
    want = ref_sparse.linear_act(None, agg, p["w"].double(), act=ACT_NAME[p["act"]])
    nan_w = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan_w), f"{what}: NaN pattern differs"
    scale = pre.abs().nan_to_num(0.0).amax(1, keepdim=True).clamp_min(1e-30)
    err = ((got.double() - want).abs() / scale)[~nan_w]
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{what}: max |got - want| / rowmax = {worst:.3e}")
    assert worst <= RTOL, f"{what}: {worst:.3e} > {RTOL}"


def _check(p, idx, what, **kw):
    idx = np.asarray(idx)
    got = _fused(p, idx, **kw)
    bad = (_bits(got) != _bits(p["h1"][torch.from_numpy(idx)])).any(1).nonzero().flatten().tolist()
    assert not bad, f"{what}: rows {bad[:8]} (pool rows {idx[bad[:8]].tolist()}, cnt {p['cnt'][idx[bad[:8]]].tolist()}) differ from the split form"
    _assert_fp64(p, idx, got, what)


def _rows(p, n, seed):
    """n pool rows: every pool row once (while they last), then at random."""
    rs = np.random.default_rng(seed)
    return np.concatenate([rs.permutation(POOL_ROWS), rs.integers(0, POOL_ROWS, max(n - POOL_ROWS, 0))])[:n]


@pytest.mark.parametrize("n_live", [1, 31, 32, 33, 63, 64, 65, 8 * 64 + 1])
def test_live_rows_around_the_tile_the_pair_and_the_eight_classes(n_live):
    p = _pool(256, 128, 15)
    _check(p, _rows(p, n_live, n_live), f"n={n_live}")


@pytest.mark.parametrize("extra", [0, 1, 32, 33])
def test_device_side_count_below_the_host_side_one(extra):
    p = _pool(256, 128, 15)
    for n_live in (64, 97):                              # the count ends a pair / ends inside tile A of one
        _check(p, _rows(p, n_live, 7 + extra), f"n={n_live} of {n_live + extra}", extra=extra)


@pytest.mark.parametrize("k", [1, 8, 9, 15, 16, 17, 64])
def test_list_lengths_around_the_request_sets(k):
    p = _pool(256, 128, k)
    _check(p, _rows(p, 97, k), f"k={k}")


@pytest.mark.parametrize("d0,h1", [(64, 128), (128, 128), (256, 32), (256, 96), (64, 32), (128, 96)])
def test_slice_counts_and_column_groups(d0, h1):
    p = _pool(d0, h1, 15)
    _check(p, _rows(p, 97, d0 + h1), f"d0={d0} h1={h1}")


def test_a_block_walks_a_second_pair():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 64 + 33
    p = _pool(64, 32, 1)
    _check(p, np.arange(n) % POOL_ROWS, f"n={n}", extra=0)


def test_empty_rows_under_both_flags():
    p = _pool(256, 128, 15, act=ops.ACT_RELU)
    idx = _rows(p, 97, 3)
    idx = idx[p["cnt"][idx] > 0]
    idx[13] = idx[50] = np.nonzero(p["cnt"] == 0)[0][0]  # one empty row in either tile of pair 0
    empty = p["cnt"][idx] == 0
    _check(p, idx, "flag=1")                             # the pool's own flag: the empty row is NaN
    for flag in (0, None):
        got = _fused(p, idx, flag=flag)
        assert (got[empty] == 0).all(), "an empty row under flag 0 is relu(0 . W)"
        assert torch.equal(_bits(got[~empty]), _bits(p["h1"][torch.from_numpy(idx[~empty])])), "the flag changed a non-empty row"


@pytest.mark.parametrize("k", [15, 25])
def test_self_rows(k):
    p = _pool(256, 128, k, self_loop=True)
    among = [(p["self"][r] == p["nbr"][r, :p["cnt"][r]]).any() for r in range(POOL_ROWS)]
    assert any(among) and not all(among), "the pool needs self rows inside and outside their lists"
    _check(p, _rows(p, 97, k), f"self rows, k={k}")


def test_same_row_at_both_pair_positions_and_two_counts():
    p = _pool(256, 128, 15)
    base = _rows(p, 97, 11)
    r = int(np.nonzero(p["cnt"] == 15)[0][0])
    a, b = base.copy(), base.copy()
    a[5], b[37] = r, r                                   # tile A / tile B of pair 0
    ga, gb = _fused(p, a), _fused(p, b)
    gc = _fused(p, b[:64])                               # another live count
    want = _bits(p["h1"][r])
    assert torch.equal(_bits(ga[5]), want) and torch.equal(_bits(gb[37]), want) and torch.equal(_bits(gc[37]), want)
    assert torch.equal(_bits(ga), _bits(_fused(p, a))), "two launches on the same inputs differ"


def _torch_mm_classes(table, w, nbr, cnt, got, what):
    """test_gpu_layer1_fused.py's special-values rule: classes as torch.mm's on the fp32 means, finite entries to RTOL of the row."""
    n, d0 = len(cnt), table.shape[1]
    mean = torch.zeros(n, d0)
    for r in range(n):
        acc = torch.zeros(d0)
        for j in range(cnt[r]):
            acc = acc + table[nbr[r, j]]
        mean[r] = acc * (torch.tensor(1.0) / float(cnt[r]))
    want = mean.mm(w.t())
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN classes differ from torch.mm"
    assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want)), f"{what}: Inf classes"
    fin = torch.isfinite(want)
    scale = want.double().abs().where(fin, torch.zeros((), dtype=torch.float64)).amax(1, keepdim=True).clamp_min(1e-30)
    err = ((got.double() - want.double()).abs() / scale)[fin]
    print(f"{what}: {int((~fin.all(1)).sum())} rows with Inf / NaN, max finite error / rowmax = {float(err.max()):.3e}")
    assert float(err.max()) <= RTOL


@pytest.mark.parametrize("where", ["first tile", "second tile", "W1"])
def test_inf_in_one_tile_of_a_pair_or_in_w1(where):
    p = _pool(256, 128, 15)
    ok = np.nonzero((p["cnt"] >= 2) & (np.abs(p["h1"].numpy()) < 1e30).all(1))[0]      # ordinary rows only: no NaN row, no 3e38 row
    idx = ok[:64]
    plain = _fused(p, idx)
    assert torch.equal(_bits(plain), _bits(p["h1"][torch.from_numpy(idx)]))
    table, w = p["table"].clone(), p["w"].clone()
    nbr, cnt = p["nbr"][idx], p["cnt"][idx]
    if where == "W1":
        w[3, 70] = float("inf")
        got = _fused(p, idx, w=w)
    else:
        row = 9 if where == "first tile" else 41
        live = np.arange(15)[None, :] < cnt[:, None]
        met = np.bincount(nbr[live], minlength=table.shape[0])
        victim = int([v for v in nbr[row, :cnt[row]] if met[v] == 1][0])      # a table row that this list alone holds
        table[victim, 100] = float("inf")
        hit = (nbr == victim) & live
        hit_rows = hit.any(1)
        lo, hi = (0, 32) if where == "first tile" else (32, 64)
        assert hit_rows[row] and not hit_rows[:lo].any() and not hit_rows[hi:].any(), "the Inf row must be met in one tile only"
        got = _fused(p, idx, table_sliced=ops.slice_major(table.to(DEV)))
        other = np.r_[0:lo, hi:64]
        assert torch.equal(_bits(got[other]), _bits(plain[other])), "the other tile of the pair lost its bits to this tile's flag"
        assert torch.equal(_bits(got[lo:hi][~hit_rows[lo:hi]]), _bits(plain[lo:hi][~hit_rows[lo:hi]])), "an ordinary row of the flagged tile changed"
    _torch_mm_classes(table, w, nbr.astype(np.int64), cnt, got, where)
