"""CPU checks of the full-neighbourhood mean's backward (sage_csr_mean_backward): argument validation before any launch, the
workspace query, ops.csr_transpose on CPU tensors, and that the whole-graph trainer's module imports without a GPU."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from sage355 import native, ops


def test_csr_mean_backward_rejects_bad_arguments_before_any_launch():
    L = native.lib()
    # every array NULL: whatever else is wrong, nothing can be launched
    args = dict(num_nodes=10, n=5, max_edges=100, ldg=4, dim=4, self_loop=0, ldgt=4)

    def call(**kw):
        a = dict(args, **kw)
        return L.sage_csr_mean_backward(None, None, None, None, a["num_nodes"], None, a["n"], a["max_edges"], None, a["ldg"], a["dim"],
                                        a["self_loop"], None, a["ldgt"], None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(dim=0), b"dim"), (dict(ldg=3), b"ldg"), (dict(ldgt=2), b"ldgt"), (dict(n=-1), b"n ="),
                     (dict(n=11), b"node list"), (dict(num_nodes=-1), b"num_nodes"), (dict(max_edges=-1), b"max_edges"),
                     (dict(self_loop=2), b"self_loop"), (dict(self_loop=-1), b"self_loop")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())


def test_csr_mean_backward_workspace_is_checked_before_any_launch():
    """Arrays that are not NULL (host memory: nothing may be launched on them), then a short, a missing and a misaligned workspace;
    with n == 0 and a good workspace the call returns SAGE_OK without a launch."""
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    need = L.sage_csr_mean_backward_workspace_bytes(10, 5, 100, 4)
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    def call(ws, nbytes, n=5):
        return L.sage_csr_mean_backward(p, p, p, p, 10, None, n, 100, p, 4, 4, 0, p, 4, ctypes.c_void_p(ws), nbytes, None)

    assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert call(None, need) == native.ENOSPACE
    assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
    need0 = L.sage_csr_mean_backward_workspace_bytes(10, 0, 100, 4)
    assert call(base, need0, n=0) == 0


def test_csr_mean_backward_workspace_query():
    L = native.lib()
    ws = L.sage_csr_mean_backward_workspace_bytes
    assert ws(-1, 0, 10, 4) == 0 and ws(10, -1, 10, 4) == 0 and ws(10, 10, -1, 4) == 0 and ws(10, 10, 10, 0) == 0
    assert ws(1 << 31, 10, 10, 4) == 0
    for nn in (0, 1, 100, 2049, 1 << 20):
        for n in (0, 1, 100, 2048, 2049, 1 << 20):
            for e in (0, 511, 512, 513, 10_000, 30_000_000):
                for d in (1, 3, 50, 256):
                    b = ws(nn, n, e, d)
                    assert b > 0 and b % 256 == 0, (nn, n, e, d, b)
                    assert ws(nn + 1, n, e, d) >= b and ws(nn, n + 1, e, d) >= b and ws(nn, n, e + 1, d) >= b and ws(nn, n, e, d + 1) >= b, \
                        (nn, n, e, d)
    # the partial sums: one [dim] row per chunk of a row longer than the chunk; the weights: a float and a flag per node
    assert native.CSR_MEAN_CHUNK == 512
    assert ws(1, 1, 100 * 512, 256) - ws(1, 1, 0, 256) >= 100 * 256 * 4
    assert ws(1 << 20, 1, 0, 4) - ws(64, 1, 0, 4) >= ((1 << 20) - 64) * 8


def _random_csr(seed, n=300, max_deg=9):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, max_deg, n)
    deg[rng.random(n) < 0.2] = 0                                   # empty rows
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    col[1::5] = col[0::5][: len(col[1::5])]                        # duplicate entries (inside a row wherever both fall in one)
    return rowptr, col


def test_csr_transpose_matches_numpy():
    rowptr, col = _random_csr(0)
    n = len(rowptr) - 1
    rp_t, c_t = ops.csr_transpose(torch.from_numpy(rowptr), torch.from_numpy(col))
    assert rp_t.dtype == torch.int64 and c_t.dtype == torch.int32 and rp_t.shape == (n + 1,) and c_t.shape == col.shape
    src = np.repeat(np.arange(n), np.diff(rowptr))
    rows = [[] for _ in range(n)]
    for v, u in zip(src, col):                                     # (v -> u) in CSR order: v ascending
        rows[u].append(v)
    assert np.array_equal(rp_t.numpy(), np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
    assert np.array_equal(c_t.numpy(), np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]))
    for u in range(n):                                             # ascending sources inside a row, duplicates kept
        r = c_t.numpy()[rp_t[u]:rp_t[u + 1]]
        assert np.all(np.diff(r) >= 0)
    assert any(len(r) != len(set(r)) for r in rows), "the test graph holds no duplicate entry"


def test_csr_transpose_twice_is_the_graph_with_sorted_rows():
    rowptr, col = _random_csr(1)
    rp_t, c_t = ops.csr_transpose(torch.from_numpy(rowptr), torch.from_numpy(col))
    rp_tt, c_tt = ops.csr_transpose(rp_t, c_t)
    assert np.array_equal(rp_tt.numpy(), rowptr)
    want = np.concatenate([np.sort(col[rowptr[v]:rowptr[v + 1]]) for v in range(len(rowptr) - 1)])
    assert np.array_equal(c_tt.numpy(), want)
    # a graph without nodes or edges
    rp0, c0 = ops.csr_transpose(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert rp0.tolist() == [0, 0, 0, 0] and c0.numel() == 0


def test_csr_transpose_refuses_ids_outside_the_graph():
    rowptr, col = _random_csr(2)
    for bad in (-1, len(rowptr) - 1):
        c = col.copy()
        c[7] = bad
        with pytest.raises(native.SageError):
            ops.csr_transpose(torch.from_numpy(rowptr), torch.from_numpy(c))


def test_fullgraph_module_imports_without_gpu():
    mod = importlib.import_module("sage355.fullgraph")
    for name in ("FullGraphTrainer", "run_full_graph_training"):
        assert callable(getattr(mod, name))
    from sage355 import autograd
    assert callable(autograd.csr_mean) and callable(ops.csr_mean_backward) and callable(ops.csr_mean_backward_workspace_bytes)
