"""CPU checks of the indexed full-neighbourhood mean (sage_csr_mean_indexed) and the grouped backward
(sage_csr_mean_backward_grouped): the symbols, argument validation before any launch, the workspace query, and
ops.csr_transpose_grouped on CPU tensors against a brute-force construction."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = native.CSR_MEAN_CHUNK
NEW = ("sage_csr_mean_indexed", "sage_csr_mean_backward_grouped", "sage_csr_mean_backward_grouped_workspace_bytes")


def test_the_new_entries_are_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert L.sage_csr_mean_backward_grouped_workspace_bytes.restype is ctypes.c_size_t
    assert L.sage_csr_mean_indexed.restype is ctypes.c_int32 and L.sage_csr_mean_backward_grouped.restype is ctypes.c_int32
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9


def test_csr_mean_indexed_rejects_bad_arguments_before_any_launch():
    L = native.lib()
    args = dict(num_nodes=10, n=10, max_edges=100, embed_rows=7, ld=4, dim=4, self_loop=0, ldo=4)

    def call(**kw):                                               # every array NULL: whatever else is wrong, nothing can be launched
        a = dict(args, **kw)
        return L.sage_csr_mean_indexed(None, None, a["num_nodes"], None, a["n"], a["max_edges"], None, None, a["embed_rows"], a["ld"],
                                       a["dim"], a["self_loop"], None, None, a["ldo"], None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(dim=0), b"dim"), (dict(dim=-3), b"dim"), (dict(ld=3), b"ld ="), (dict(ldo=2), b"ldo"), (dict(num_nodes=-1), b"num_nodes"),
                     (dict(num_nodes=1 << 31), b"num_nodes"), (dict(n=-1), b"n ="), (dict(n=11), b"without a node list"),
                     (dict(max_edges=-1), b"max_edges"), (dict(embed_rows=0), b"embed_rows"), (dict(embed_rows=1 << 31), b"embed_rows"),
                     (dict(self_loop=2), b"self_loop")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())


def test_csr_mean_backward_grouped_rejects_bad_arguments_before_any_launch():
    L = native.lib()
    args = dict(num_nodes=10, num_groups=6, max_edges=100, ldg=4, dim=4, self_loop=0, ldge=4)

    def call(**kw):
        a = dict(args, **kw)
        return L.sage_csr_mean_backward_grouped(None, None, None, None, a["num_nodes"], a["num_groups"], a["max_edges"], None, a["ldg"],
                                                a["dim"], a["self_loop"], None, a["ldge"], None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(dim=0), b"dim"), (dict(ldg=3), b"ldg"), (dict(ldge=2), b"ldge"), (dict(num_nodes=-1), b"num_nodes"),
                     (dict(num_nodes=1 << 31), b"num_nodes"), (dict(num_nodes=0), b"num_nodes"), (dict(num_groups=-1), b"num_groups"),
                     (dict(num_groups=1 << 31), b"num_groups"), (dict(max_edges=-1), b"max_edges"), (dict(self_loop=-1), b"self_loop")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())


def test_the_workspace_is_checked_before_any_launch():
    """Arrays that are not NULL (host memory: nothing may be launched on them), then a short, a missing and a misaligned workspace;
    with no rows and a good workspace the calls return SAGE_OK without a launch."""
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    need_f = L.sage_csr_mean_workspace_bytes(10, 5000, 4)
    need_b = L.sage_csr_mean_backward_grouped_workspace_bytes(10, 6, 5000, 4)
    assert need_f > 0 and need_b > 0
    buf = (ctypes.c_char * (max(need_f, need_b) + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    def fwd(ws, nbytes, n=10, max_edges=5000):
        return L.sage_csr_mean_indexed(p, p, 10, None, n, max_edges, p, p, 7, 4, 4, 1, None, p, 4, ctypes.c_void_p(ws), nbytes, None)

    def bwd(ws, nbytes, groups=6, max_edges=5000):
        return L.sage_csr_mean_backward_grouped(p, p, p, p, 10, groups, max_edges, p, 4, 4, 1, p, 4, ctypes.c_void_p(ws), nbytes, None)

    for call, need in ((fwd, need_f), (bwd, need_b)):
        assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
        assert call(base, 0) == native.ENOSPACE
        assert call(None, need) == native.ENOSPACE
        assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
        assert call(base, need, max_edges=1 << 50) == native.EINVAL and b"out of range" in L.sage_last_error()
    assert fwd(base, L.sage_csr_mean_workspace_bytes(0, 5000, 4), n=0) == 0
    assert bwd(base, L.sage_csr_mean_backward_grouped_workspace_bytes(10, 0, 5000, 4), groups=0) == 0


def test_the_grouped_workspace_query_is_host_arithmetic():
    ws = native.lib().sage_csr_mean_backward_grouped_workspace_bytes
    assert ws(-1, 10, 10, 4) == 0 and ws(10, -1, 10, 4) == 0 and ws(10, 10, -1, 4) == 0 and ws(10, 10, 10, 0) == 0
    assert ws(1 << 31, 10, 10, 4) == 0 and ws(10, 1 << 31, 10, 4) == 0
    for n in (1, 100, 5000):
        for k in (0, 1, 2049):
            for e in (0, 512, 513, 30_000_000):
                for d in (1, 50, 256):
                    b = ws(n, k, e, d)
                    assert b > 0 and b % 256 == 0, (n, k, e, d, b)
                    assert ws(n + 1, k, e, d) >= b and ws(n, k + 1, e, d) >= b and ws(n, k, e + 1, d) >= b and ws(n, k, e, d + 1) >= b
                    # with as many rows as nodes it is the backward's own layout
                    assert ws(n, n, e, d) == native.lib().sage_csr_mean_backward_workspace_bytes(n, n, e, d)
    assert ws(10, 1, 100 * 512, 256) - ws(10, 1, 0, 256) >= 100 * 256 * 4          # one partial row per chunk of a long row
    assert ops.csr_mean_backward_grouped_workspace_bytes(10, 1, 100 * 512, 256) == ws(10, 1, 100 * 512, 256)


# ------------------------------------------------------------------------------------------------ csr_transpose_grouped
def skewed_graph(seed=0):
    """The generator of tests/test_gpu_csr_mean_backward.py: rows of degree 0, 1, E-1, E, E+1, 2E, 2E+1 and one star hub of
    20E + 37, among rows of 0..6 edges; some rows hold their own node, neighbour lists unsorted."""
    rng = np.random.default_rng(seed)
    n = 24 * E
    special = {0: 0, 1: 1, 2: E - 1, 3: E, 4: E + 1, 5: 2 * E, 6: 2 * E + 1, 7: 20 * E + 37, 8: E + 1, 9: 2 * E + 1}
    deg = rng.integers(0, 7, n)
    for v, d in special.items():
        deg[v] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    col[rowptr[7]:rowptr[8]] = rng.permutation(n)[: deg[7]]
    for v in (3, 8, 9, 20, 21, 22):
        if deg[v] > 0:
            col[rowptr[v + 1] - 1] = v
    col[rowptr[7] + 5 * E + 3] = 7
    return rowptr, col


def sym_graph():
    rowptr, col = skewed_graph()
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n), np.diff(rowptr))
    s = np.concatenate([src, col.astype(np.int64)])
    d = np.concatenate([col.astype(np.int64), src])
    order = np.argsort(s, kind="stable")
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(s, minlength=n), out=rp[1:])
    return rp, d[order].astype(np.int32)


def brute_force_grouped(rowptr, col, index, k, self_loop):
    """Part by part in Python: the transposed rows (sources ascending, duplicates kept), each node's self entry after them, the
    nodes of a group in ascending order."""
    n = len(rowptr) - 1
    t_rows = [[] for _ in range(n)]
    own = [False] * n
    for v in range(n):
        for u in col[rowptr[v]:rowptr[v + 1]].tolist():
            t_rows[u].append(v)
            own[v] |= u == v
    groups = [[] for _ in range(k)]
    for u in range(n):
        groups[int(index[u])].extend(t_rows[u])
        if self_loop and not own[u]:
            groups[int(index[u])].append(u)
    rp = np.zeros(k + 1, dtype=np.int64)
    np.cumsum([len(g) for g in groups], out=rp[1:])
    return rp, np.fromiter((x for g in groups for x in g), dtype=np.int32, count=int(rp[-1]))


@pytest.fixture(scope="module")
def sym():
    rp, col = sym_graph()
    assert len(rp) - 1 == 12_288
    return rp, col


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("kind", ["identity", "degree", "zero", "mod7"])
def test_csr_transpose_grouped_against_brute_force(sym, kind, self_loop):
    rp, col = sym
    n = len(rp) - 1
    deg = np.diff(rp)
    index, k = {"identity": (np.arange(n), n), "degree": (deg, int(deg.max()) + 1), "zero": (np.zeros(n, dtype=np.int64), 1),
                "mod7": (np.arange(n) % 7, 7)}[kind]
    want_rp, want_col = brute_force_grouped(rp, col, index, k, self_loop)
    for dtype in (torch.int32, torch.int64):
        g = ops.csr_transpose_grouped(torch.from_numpy(rp), torch.from_numpy(col), torch.from_numpy(index).to(dtype), k, self_loop=self_loop)
        assert isinstance(g, ops.GroupedTranspose) and g.self_loop is self_loop and len(g) == 3
        assert g.rowptr.dtype == torch.int64 and g.col.dtype == torch.int32 and g.rowptr.shape == (k + 1,)
        assert np.array_equal(g.rowptr.numpy(), want_rp) and np.array_equal(g.col.numpy(), want_col)
    lengths = np.diff(want_rp)
    if kind == "identity" and not self_loop:                       # exactly the transposed rows
        rp_t, c_t = ops.csr_transpose(torch.from_numpy(rp), torch.from_numpy(col))
        assert torch.equal(g.rowptr, rp_t) and torch.equal(g.col, c_t)
    if kind == "degree":                                           # the shapes the GPU tests rely on
        # empty rows: degrees nobody has; with self_loop the nodes of degree 0 put themselves into row 0
        assert (lengths == 0).sum() == (10_256 if self_loop else 10_257)
        assert ((lengths > E) & (lengths <= 2 * E)).any() and (lengths > 2 * E).sum() == 17
        assert lengths.max() == (14_378 if self_loop else 12_942)
    if kind == "zero":
        assert lengths.tolist() == [116_828 if self_loop else 104_554]


def test_csr_transpose_grouped_refuses_what_it_cannot_group():
    rp = torch.tensor([0, 2, 3, 3, 5])
    col = torch.tensor([1, 3, 0, 2, 2], dtype=torch.int32)
    good = torch.tensor([0, 2, 2, 1], dtype=torch.int32)
    g = ops.csr_transpose_grouped(rp, col, good, 3, self_loop=True)
    assert g.rowptr.tolist() == [0, 2, 4, 9] and g.col.tolist() == [1, 0, 0, 3, 0, 1, 3, 3, 2]
    for bad in (-1, 3, 1 << 20):
        idx = good.clone()
        idx[2] = bad
        with pytest.raises(native.SageError):
            ops.csr_transpose_grouped(rp, col, idx, 3)
    with pytest.raises(native.SageError):
        ops.csr_transpose_grouped(rp, col, good[:3], 3)            # len(index) != N
    with pytest.raises(native.SageError):
        ops.csr_transpose_grouped(rp, col, good.float(), 3)        # not an integer index
    for bad in (-1, 4):
        c = col.clone()
        c[1] = bad
        with pytest.raises(native.SageError):
            ops.csr_transpose_grouped(rp, c, good, 3)              # a node id outside the graph
    e = ops.csr_transpose_grouped(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 4)
    assert e.rowptr.tolist() == [0, 0, 0, 0, 0] and e.col.numel() == 0


def test_the_indexed_entry_points_import_without_gpu():
    import inspect

    from sage355 import autograd, fullgraph, inference
    assert "index" in inspect.signature(ops.csr_mean).parameters and callable(ops.csr_mean_backward_grouped)
    assert {"index", "grouped"} <= set(inspect.signature(autograd.csr_mean).parameters)
    assert "index" in inspect.signature(inference.embed_all_nodes).parameters and "index" in inspect.signature(inference.layer_all_nodes).parameters
    for fn in (fullgraph.FullGraphTrainer.__init__, fullgraph.run_full_graph_training):
        assert inspect.signature(fn).parameters["fused_embed"].default is False
