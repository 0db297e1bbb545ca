"""The phase-sliced layer 1 (csrc/sage_layer1_phase.hip: gather + contraction of the gcn encoder in one launch on the slice-major table).

Called directly through sage_layer1_fused against the fp64 oracle (ref_sparse.gather_mean then ref_sparse.linear_act on the same lists) at
its edge shapes; tolerance |got - want| <= 1e-5 * max|pre-activation row|, NaN patterns equal.  A tile is 32 rows and tiles are dealt
to 8 classes, so the row counts sit around 32 and 8 * 32.  Bit for bit: a row's result does not depend on the row count or on where the
row sits, a launch repeats itself, and -- in a child process with SAGE_LAYER1_FUSED=1, whatever the library's default is -- the engine's
one-launch form equals its gather + contraction form, the role pipeline equals the single forward, and a training engine keeps the
two-launch form (it leaves the means in the workspace).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_sparse
from sage355 import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5
SENTINEL = -31.5
ACT = {"relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lists(rs, n, k, rows, empty=0.1):
    """nbr [n, k] (distinct ids per row, -1 past cnt), cnt [n]: a mix of empty rows, short lists and full ones."""
    cnt = rs.integers(1, k + 1, n)
    cnt[rs.random(n) < 0.4] = k
    cnt[rs.random(n) < empty] = 0
    nbr = np.full((n, k), -1, np.int32)
    for r in range(n):
        nbr[r, :cnt[r]] = rs.choice(rows, cnt[r], replace=False)
    return nbr, cnt.astype(np.int32)


def _run(table, w, nbr, cnt, act, n_live, self_row=None, flag=1, cap_extra=40):
    """The kernel on the first n_live of n + cap_extra rows (device-side count); -> rows [0, n_live), and asserts the rest untouched."""
    n, k = nbr.shape
    cap = n + cap_extra
    nbr_d = torch.full((cap, k), -1, dtype=torch.int32)
    nbr_d[:n] = torch.from_numpy(nbr)
    cnt_d = torch.zeros(cap, dtype=torch.int32)
    cnt_d[:n] = torch.from_numpy(cnt)
    sr = None
    if self_row is not None:
        sr = torch.full((cap,), -1, dtype=torch.int32)
        sr[:n] = torch.from_numpy(self_row)
        sr = sr.to(DEV)
    out = torch.full((cap, w.shape[0] + 4), SENTINEL, device=DEV)[:, :w.shape[0]]
    n_dev = torch.tensor([n_live], dtype=torch.int32, device=DEV)
    any_ne = None if flag is None else torch.tensor([flag], dtype=torch.int32, device=DEV)
    ops.layer1_fused(ops.slice_major(table.to(DEV)), nbr_d.to(DEV), cnt_d.to(DEV), w.to(DEV), act=act, self_row=sr, any_nonempty=any_ne,
                     n_dev=n_dev, out=out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[n_live:] == SENTINEL).all(), "rows at or past the device-side count were written"
    return got[:n_live]


def _oracle(table, w, nbr, cnt, act, self_row=None, flag=1):
    agg = ref_sparse.gather_mean(table.double(), nbr, cnt, self_idx=self_row, nan_empty=True)
    if self_row is None:                 # an empty row's value comes from the flag the kernel was given, not from the batch
        agg[torch.from_numpy(cnt == 0)] = float("nan") if flag else 0.0
    pre = agg.mm(w.double().t())
    return ref_sparse.linear_act(None, agg, w.double(), act=act), pre


def _assert_close(got, want, pre, what):
    nan_w = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan_w), f"{what}: NaN pattern differs"
    scale = pre.abs().nan_to_num(0.0).amax(1, keepdim=True).clamp_min(1e-30)
    err = ((got.double() - want).abs() / scale)[~nan_w]
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{what}: max |got - want| / rowmax = {worst:.3e}")
    assert worst <= RTOL, f"{what}: {worst:.3e} > {RTOL}"


CASES = [
    # d0, h1, k, act, self-loop term
    (256, 128, 15, "relu", False),
    (256, 128, 25, "sigmoid", True),      # k above 16: two trips per row
    (256, 32, 15, "sigmoid", False),
    (64, 32, 1, "relu", False),           # two slices, one column group, k = 1
    (64, 128, 5, "relu", True),
    (128, 64, 10, "relu", False),
]


@pytest.mark.parametrize("d0,h1,k,act,self_loop", CASES)
@pytest.mark.parametrize("n_live", [1, 31, 33, 255, 257])
def test_fused_layer1_matches_fp64(d0, h1, k, act, self_loop, n_live):
    rs = np.random.default_rng(d0 + 7 * h1 + 13 * k + n_live)
    gen = torch.Generator().manual_seed(d0 + h1 + k + n_live)
    rows = 401
    table = torch.randn(rows, d0, generator=gen)
    w = torch.randn(h1, d0, generator=gen) / np.sqrt(d0)
    nbr, cnt = _lists(rs, n_live, k, rows)
    self_row = None
    if self_loop:
        self_row = rs.integers(0, rows, n_live).astype(np.int32)
        hit = rs.random(n_live) < 0.3                           # the row's own id is already among its neighbours: counted once
        self_row[hit & (cnt > 0)] = nbr[hit & (cnt > 0), 0]
    got = _run(table, w, nbr, cnt, ACT[act], n_live, self_row=self_row)
    want, pre = _oracle(table, w, nbr, cnt, act, self_row=self_row)
    _assert_close(got, want, pre, f"d0={d0} h1={h1} k={k} {act} self={self_loop} n={n_live}")


def test_no_rows_and_all_empty_batch():
    gen = torch.Generator().manual_seed(3)
    table, w = torch.randn(100, 256, generator=gen), torch.randn(128, 256, generator=gen) / 16
    nbr = np.full((40, 15), -1, np.int32)
    cnt = np.zeros(40, np.int32)
    assert _run(table, w, nbr, cnt, ops.ACT_RELU, 0).shape[0] == 0            # s1_count = 0: nothing written (asserted inside)
    got = _run(table, w, nbr, cnt, ops.ACT_RELU, 40, flag=0)                  # an all-empty batch: zero means, relu(0) = 0
    assert (got == 0).all()
    got = _run(table, w, nbr, cnt, ops.ACT_SIGMOID, 40, flag=None)            # no flag at all: zeros too, sigmoid(0) = 0.5
    assert (got == 0.5).all()
    cnt[:5] = 1
    nbr[:5, 0] = 7
    got = _run(table, w, nbr, cnt, ops.ACT_RELU, 40, flag=1)                  # a mixed batch: the empty rows are NaN (reference 0/0)
    assert torch.isnan(got[5:]).all() and not torch.isnan(got[:5]).any()


def test_special_values_follow_torch_mm():
    """Inf / NaN / 2^126-magnitude table entries: the rows that meet them take the exact fp32 chain; classes as torch.mm's on the fp32 means."""
    gen = torch.Generator().manual_seed(11)
    rs = np.random.default_rng(11)
    rows, d0, h1, k, n = 300, 256, 128, 15, 97
    table = torch.randn(rows, d0, generator=gen)
    table[10, 3] = float("inf")
    table[11, 200] = float("-inf")
    table[12, 77] = float("nan")
    table[13, 130] = 2.0 ** 126
    table[14, 255] = -(2.0 ** 127)
    w = torch.randn(h1, d0, generator=gen) / 16
    nbr, cnt = _lists(rs, n, k, rows, empty=0.0)
    for i, special in enumerate((10, 11, 12, 13, 14)):
        if special not in nbr[3 * i, :cnt[3 * i]]:
            nbr[3 * i, 0] = special
    got = _run(table, w, nbr, cnt, ops.ACT_NONE, n)
    mean = torch.zeros(n, d0)
    for r in range(n):
        acc = torch.zeros(d0)
        for j in range(cnt[r]):
            acc = acc + table[nbr[r, j]]
        mean[r] = acc * (torch.tensor(1.0) / float(cnt[r]))
    want = mean.mm(w.t())
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN classes differ from torch.mm"
    assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want)), "Inf classes differ"
    fin = torch.isfinite(want)
    rows_ok = fin.all(1)
    scale = want.double().abs().where(fin, torch.zeros((), dtype=torch.float64)).amax(1, keepdim=True).clamp_min(1e-30)
    err = ((got.double() - want.double()).abs() / scale)[fin]
    print(f"special values: {int((~rows_ok).sum())} rows with Inf / NaN, max finite error / rowmax = {float(err.max()):.3e}")
    assert float(err.max()) <= RTOL


def test_row_bits_do_not_depend_on_position_or_count():
    gen = torch.Generator().manual_seed(5)
    rs = np.random.default_rng(5)
    rows, d0, h1, k, n = 500, 256, 128, 15, 300
    table, w = torch.randn(rows, d0, generator=gen), torch.randn(h1, d0, generator=gen) / 16
    nbr, cnt = _lists(rs, n, k, rows)
    a = _run(table, w, nbr, cnt, ops.ACT_RELU, n)
    b = _run(table, w, nbr, cnt, ops.ACT_RELU, n)
    assert torch.equal(_bits(a), _bits(b)), "two launches on the same inputs differ"
    perm = rs.permutation(n)[:77]                                           # other tile, other class, other row count
    c = _run(table, w, nbr[perm], cnt[perm], ops.ACT_RELU, 77)
    assert torch.equal(_bits(c), _bits(a[torch.from_numpy(perm)])), "a row's bits depend on where it sits"


_CHILD = r"""
import numpy as np, torch
from sage355 import native
from sage355.engine import TwoHopEngine, RolePipeline
from sage355.graph import rmat_graph
from sage355.train import EngineTrainer

g = rmat_graph(12, 60_000, seed=1)
gen = torch.Generator().manual_seed(0)
d0, h1, h2, k1, k2, b = 256, 128, 128, 15, 25, 512
table = torch.randn(g.num_nodes, d0, generator=gen).cuda()
w1 = (torch.randn(h1, d0, generator=gen) / 16).cuda()
w2 = (torch.randn(h2, h1, generator=gen) / 11).cuda()
seeds = np.random.default_rng(0).choice(np.nonzero(g.degrees() > 0)[0], b, replace=False).astype(np.int32)
sd = torch.from_numpy(np.stack([seeds, seeds[::-1].copy(), np.roll(seeds, 7)])).cuda()
rowptr, col = g.to("cuda")
MARK = -77.25

def agg1_region(e):
    L = e.layout
    return e._view(L.agg1, L.max_s1 * e.d0p, torch.float32)

with torch.no_grad():
    eng = TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=b)
    assert eng.layout.layer1_split
    agg1_region(eng).fill_(MARK)
    out_f = eng.forward(sd[0], seed=42).clone()
    assert eng._table_sliced is not None and eng._slice_floats == 32        # (the slice-major copy is made by the first forward)
    it = eng.intermediates()
    h1_f = it["h1"][torch.argsort(it["s1_nodes"].long())].clone()          # the frontier's row order is arbitrary: compare by node id
    assert it["agg1"] is None and not eng._kept_means
    assert bool((agg1_region(eng) == MARK).all()), "the one-launch layer 1 did not run: the means were written"
    eng.keep_means = True
    out_k = eng.forward(sd[0], seed=42).clone()
    it = eng.intermediates()
    assert it["agg1"] is not None and not bool((it["agg1"] == MARK).any()), "keep_means did not leave the means in the workspace"
    h1_k = it["h1"][torch.argsort(it["s1_nodes"].long())].clone()
    assert torch.equal(h1_k.view(torch.int32), h1_f.view(torch.int32)), "h1 of the one-launch form differs from gather + contraction"
    assert torch.equal(out_k.view(torch.int32), out_f.view(torch.int32))
    eng.keep_means = False
    assert torch.equal(eng.forward(sd[0], seed=42).view(torch.int32), out_f.view(torch.int32)), "the one-launch form does not repeat itself"

    pipe = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=2, threads=True)
    assert not any(e._wants_means() for e in pipe.engines) and pipe.engines[0]._model().keep_means == 0
    for e in pipe.engines:
        agg1_region(e).fill_(MARK)
    po = torch.empty(3, b, h2, device="cuda")
    pipe.submit_many(sd, [42, 43, 44], po)
    pipe.synchronize()
    for i in range(3):
        assert torch.equal(po[i], eng.forward(sd[i], seed=42 + i)), "role pipeline differs from the single forward"
    assert all(bool((agg1_region(e) == MARK).all()) for e in pipe.engines), "the role pipeline wrote the means"

# training keeps the two-launch form
tr = EngineTrainer(rowptr, col, table, 7, hidden1=h1, hidden2=h2, num_sample1=k1, num_sample2=k2, gcn=True, max_batch=b)
e = tr.engine
assert e.keep_means and e._wants_means() and e._model(keep_means=e._wants_means()).keep_means == 1
agg1_region(e).fill_(MARK)
tr.embed(sd[0], key=1)
torch.cuda.synchronize()
assert e._kept_means and not bool((agg1_region(e)[: 64 * d0] == MARK).any()), "a training engine's forward did not leave the means"
print("CHILD OK")
"""


def test_engine_forms_agree_bit_for_bit_and_training_keeps_the_means(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    env = dict(os.environ, SAGE_LAYER1_FUSED="1",
               PYTHONPATH=os.pathsep.join([REPO, os.path.join(REPO, "graphsage-simple_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-3000:], res.stderr[-3000:])
    assert res.returncode == 0 and "CHILD OK" in res.stdout
