"""The output BITS of the six chunked row sums (sage_csr_mean / _indexed, sage_csr_sum, sage_csr_mean_backward / _grouped,
sage_embed_grad / _rows), pinned: tests/golden/chunked_sum_bits.json maps a case name to the SHA-256 of the output bytes.

The neighbouring tests hold each entry to fp64 within a bound and check that its bits do not depend on the run or on the workspace
bound; none of them would notice another association of the same terms that stays inside the bound.  This one does: the digests were
recorded from the library as it was BEFORE the chunk rule became one piece of code (csrc/sage_csr_common.h), so every later build has
to give those bits -- the chunk pass, the fall-back of a long row without workspace room and the in-place walk alike.

Inputs are the neighbours' builders: the skewed graph (rows of exactly 0, 1, E-1, E, E+1, 2E, 2E+1 and 20E+37 entries, self entries
in a last chunk), its symmetrised and its transposed form, the degree index, the group sizes of tests/test_gpu_csr_sum.py and the
term sets of tests/test_gpu_embed_grad.py / test_gpu_embed_sparse.py.  Every CSR case runs at three workspace bounds: the true entry
count (every long row in the chunk pass), 0 (every long row on the fall-back) and one between, at which the longest row misses the
item list while a row of two or three chunks fits; the three digests must be equal, and equal to the recorded one.

To record (only ever from a build of the commit BEFORE a change that must keep the bits; experiments/ab_build.sh shows the form):
    SAGE355_LIB=<that build's .so> PYTHONPATH=graphsage-simple_amd:tests python tests/test_gpu_chunked_sum_bits.py --record"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from sage355 import native, ops
from test_csr_mean_indexed_host import skewed_graph, sym_graph
import test_gpu_csr_sum as sum_inputs
import test_gpu_embed_sparse as embed_inputs

DEV = "cuda"
E = native.CSR_MEAN_CHUNK
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chunked_sum_bits.json")


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def item_cap(n, max_edges):
    """the item entries chunk_ws of csrc/sage_csr_common.h sizes a workspace for"""
    return max_edges // E + min(n, max_edges // (E + 1))


def bounds(lengths):
    """(true entry count, 0, a bound between) for rows of these lengths, in row order: at the last one the longest row's chunks miss
    the item list and those of at least one other long row fit (the first long rows: in the skewed graph the rows of E+1 and 2E entries)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    k = np.where(lengths > E, (lengths + E - 1) // E, 0)
    o = np.cumsum(k) - k
    hub = int(np.argmax(lengths))
    assert k[hub] > 3 and (k > 0).sum() >= 2
    for m in range(1, int(lengths.sum()) // E + 2):
        cap = item_cap(len(lengths), m * E)
        fits = (k > 0) & (o + k <= cap)
        if fits.any() and not fits[hub]:
            assert item_cap(len(lengths), int(lengths.sum())) >= int(k.sum()), "the true count must hold every chunk"
            return int(lengths.sum()), 0, m * E
    raise AssertionError("no workspace bound splits the long rows")


def wide(rows, dim, ld, seed):
    """[rows, dim] on the device with leading dimension ld, from a CPU generator"""
    t = torch.randn(rows, ld, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return t[:, :dim] if ld != dim else t


_graphs = {}


def graph(name):
    """"fwd": the skewed graph (forward rows of the exact lengths); "sym": with its reverse; "rev": its transpose (transposed rows of the
    exact lengths) -> dict(rowptr, col numpy; rp, cl on the device; the transpose on the device; the degree index and its row count)"""
    if name not in _graphs:
        if name == "fwd":
            rowptr, col = skewed_graph()
        elif name == "sym":
            rowptr, col = sym_graph()
        else:
            rp_t, c_t = ops.csr_transpose(*(torch.from_numpy(a) for a in skewed_graph()))
            rowptr, col = rp_t.numpy(), c_t.numpy()
        rp, cl = torch.from_numpy(rowptr), torch.from_numpy(col)
        rp_t, c_t = ops.csr_transpose(rp, cl)
        deg = np.diff(rowptr)
        _graphs[name] = dict(rowptr=rowptr, col=col, n=len(rowptr) - 1, deg=deg, deg_t=np.diff(rp_t.numpy()), rp=rp.to(DEV), cl=cl.to(DEV),
                             rp_t=rp_t.to(DEV), c_t=c_t.to(DEV), index=torch.from_numpy(deg.astype(np.int32)).to(DEV), groups=int(deg.max()) + 1,
                             grouped={})
    return _graphs[name]


# ---------------------------------------------------------------------------------------------- csr_mean and csr_mean(index=)
MEAN_WIDTHS = [(4, 4), (260, 260), (7, 10), (67, 70)]           # (dim, ld): vec4 below and across the 256-column trip; scalar, 64-column


def mean_case(indexed, self_loop, subset, dim, ld):
    def run():
        g = graph("fwd")
        n = g["n"]
        if subset:                                                # rows of two and three chunks, the hub twice, ids outside the graph, random rows
            ids = np.concatenate([[4, 5, 6, 3, 7, 7, -1, n, 0, 9, 9, n - 1, 1 << 30], np.random.default_rng(3).integers(0, n, 300)])
            lengths = np.where((ids >= 0) & (ids < n), g["deg"][np.clip(ids, 0, n - 1)], 0)
            kw = dict(nodes=torch.from_numpy(ids.astype(np.int32)).to(DEV))
        else:
            lengths, kw = g["deg"], {}
        if indexed:
            table, kw["index"] = wide(g["groups"], dim, ld, seed=dim), g["index"]
        else:
            table = wide(n, dim, ld, seed=dim)
        flag = torch.ones(1, dtype=torch.int32, device=DEV)
        return [digest(ops.csr_mean(g["rp"], g["cl"], table, self_loop=bool(self_loop), any_nonempty=flag, max_edges=m, **kw))
                for m in bounds(lengths)]
    return run


# ---------------------------------------------------------------------------------------------- csr_sum
def sum_case(dim):
    def run():
        rowptr = np.concatenate([[0], np.cumsum(sum_inputs.SIZES)]).astype(np.int64)
        col = np.random.default_rng(7).permutation(sum_inputs.N).astype(np.int32)     # tests/test_gpu_csr_sum.py's grouping
        rp, cl = torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV)
        table = sum_inputs.table_of(dim).to(DEV)
        return [digest(ops.csr_sum(rp, cl, table, max_edges=m)) for m in bounds(sum_inputs.SIZES)]
    return run


# ---------------------------------------------------------------------------------------------- csr_mean_backward and _grouped
def backward_case(grouped, name, self_loop, dim):
    def run():
        g = graph(name)
        grad = wide(g["n"], dim, dim, seed=100 + dim)
        if not grouped:
            return [digest(ops.csr_mean_backward(g["rp"], g["cl"], g["rp_t"], g["c_t"], grad, self_loop=bool(self_loop), max_edges=m))
                    for m in bounds(g["deg_t"])]
        if self_loop not in g["grouped"]:
            g["grouped"][self_loop] = ops.csr_transpose_grouped(g["rp"], g["cl"], g["index"], g["groups"], self_loop=bool(self_loop))
        gt = g["grouped"][self_loop]
        return [digest(ops.csr_mean_backward_grouped(g["rp"], g["cl"], gt, grad, max_edges=m)) for m in bounds(np.diff(gt.rowptr.cpu().numpy()))]
    return run


# ---------------------------------------------------------------------------------------------- embed_grad and embed_grad_rows
EMBED_WIDTHS = [8, 64, 128, 256]                                  # one per lane-group size: 8, 16, 32 and 64 lanes
EMBED_FANOUTS = [7, 64]                                           # embed_inputs.SIZES: runs of no term, of one chunk and of up to six
EMBED_ROWS = 1 << 12                                              # the 15 ids spread over this many embedding rows


def spread(nbr):
    """embed_inputs.id_map's placement at EMBED_ROWS rows: increasing, ids 0 and EMBED_ROWS - 1 images of run-less ids; padding stays -1"""
    m = np.arange(embed_inputs.R, dtype=np.int64) * ((EMBED_ROWS - 1) // (embed_inputs.R + 1))
    m[-1], m[-2] = EMBED_ROWS - 1, EMBED_ROWS - 2
    assert m[0] == 0 and np.all(np.diff(m) > 0)
    return np.where(nbr >= 0, m[np.maximum(nbr, 0)], -1).astype(np.int32)


def embed_sets(k, ordered):
    """(nbr, cnt on the device, keyword arguments): as the sets lie, or in ops.row_order's order with a third of them dead"""
    nodes, nbr, cnt = embed_inputs.case(k)
    nodes_d, nbr_d, cnt_d = embed_inputs.dev(nodes, spread(nbr), cnt)
    if not ordered:
        return nbr_d, cnt_d, {}
    n = len(cnt)
    n_dev = torch.tensor([n - n // 3], dtype=torch.int32, device=DEV)
    return nbr_d, cnt_d, dict(n_dev=n_dev, row_order=ops.row_order(nodes_d, n_dev=n_dev))


def embed_case(kind, k, dim, ordered):
    def run():
        rows_n = EMBED_ROWS
        nbr_d, cnt_d, kw = embed_sets(k, ordered)
        g = embed_inputs.grad_of(k, dim).to(DEV)
        if kind == "dense":
            return [digest(ops.embed_grad(g, nbr_d, cnt_d, rows_n, **kw))]
        if kind == "rows":
            rows, num, grad = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, **kw)
            u = int(num)
            assert 0 < u <= embed_inputs.NU
            return [digest(num, rows[:u], grad[:u])]
        table = torch.randn(rows_n, dim, generator=torch.Generator().manual_seed(7)).to(DEV)
        _, num, _ = ops.embed_grad_rows(g, nbr_d, cnt_d, rows_n, embed=table, lr=0.7, want_grad=False, **kw)
        assert int(num) > 0
        return [digest(num, table)]
    return run


CASES = {}
for _indexed in (False, True):
    for _sl in (0, 1):
        for _subset in (False, True):
            for _dim, _ld in MEAN_WIDTHS:
                CASES[f"csr_mean{'_indexed' if _indexed else ''}-self{_sl}-{'subset' if _subset else 'all'}-dim{_dim}-ld{_ld}"] = \
                    mean_case(_indexed, _sl, _subset, _dim, _ld)
for _dim in (4, 260, 7):
    CASES[f"csr_sum-dim{_dim}"] = sum_case(_dim)
for _grouped in (False, True):
    for _name in ("sym", "rev"):
        for _sl in (0, 1):
            for _dim in (4, 260, 7):
                CASES[f"csr_mean_backward{'_grouped' if _grouped else ''}-{_name}-self{_sl}-dim{_dim}"] = backward_case(_grouped, _name, _sl, _dim)
for _kind in ("dense", "rows", "update"):
    for _k in EMBED_FANOUTS:
        for _dim in EMBED_WIDTHS:
            for _ordered in (False, True):
                CASES[f"embed_grad{'' if _kind == 'dense' else '_rows-' + _kind}-k{_k}-dim{_dim}-{'ordered' if _ordered else 'plain'}"] = \
                    embed_case(_kind, _k, _dim, _ordered)


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded_and_nothing_else():
    assert sorted(recorded()) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_bits_are_the_recorded_ones(name):
    got = CASES[name]()
    assert len(set(got)) == 1, f"{name}: the bits depend on the workspace bound: {got}"
    assert got[0] == recorded()[name], f"{name}: SHA-256 {got[0]}, recorded {recorded()[name]}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    out = {}
    for case_name in sorted(CASES):
        got = CASES[case_name]()
        assert len(set(got)) == 1, f"{case_name}: the bits depend on the workspace bound: {got}"
        out[case_name] = got[0]
        print(case_name, got[0], flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} digests from {native.LIB_PATH} -> {GOLDEN}")
