"""CPU checks of the grouped row sum (sage_csr_sum): the symbol, argument validation before any launch, the workspace query, and
ops.group_rows on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_csr_sum_is_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in ("sage_csr_sum", "sage_csr_sum_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
    assert L.sage_csr_sum_workspace_bytes.restype is ctypes.c_size_t
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9


def test_csr_sum_rejects_bad_arguments_before_any_launch():
    L = native.lib()
    args = dict(num_rows=10, max_edges=100, table_rows=7, ld=4, dim=4, ldo=4)

    def call(**kw):                                               # every array NULL: whatever else is wrong, nothing can be launched
        a = dict(args, **kw)
        return L.sage_csr_sum(None, None, a["num_rows"], a["max_edges"], None, a["table_rows"], a["ld"], a["dim"], None, a["ldo"], None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(dim=0), b"dim"), (dict(dim=-3), b"dim"), (dict(ld=3), b"ld ="), (dict(ldo=2), b"ldo"), (dict(num_rows=-1), b"num_rows"),
                     (dict(num_rows=1 << 31), b"num_rows"), (dict(max_edges=-1), b"max_edges"), (dict(table_rows=0), b"table_rows"),
                     (dict(table_rows=1 << 31), b"table_rows"), (dict(max_edges=1 << 50), b"out of range")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())


def test_csr_sum_workspace_is_checked_before_any_launch():
    """Arrays that are not NULL (host memory: nothing may be launched on them), then a short, a missing and a misaligned workspace;
    with num_rows == 0 and a good workspace the call returns SAGE_OK without a launch."""
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    need = L.sage_csr_sum_workspace_bytes(10, 5000, 4)
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    def call(ws, nbytes, num_rows=10):
        return L.sage_csr_sum(p, p, num_rows, 5000, p, 7, 4, 4, p, 4, ctypes.c_void_p(ws), nbytes, None)

    assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert call(base, 0) == native.ENOSPACE
    assert call(None, need) == native.ENOSPACE
    assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
    assert call(base, L.sage_csr_sum_workspace_bytes(0, 5000, 4), num_rows=0) == 0


def test_csr_sum_workspace_query_is_host_arithmetic():
    ws = native.lib().sage_csr_sum_workspace_bytes
    assert ws(-1, 10, 4) == 0 and ws(10, -1, 4) == 0 and ws(10, 10, 0) == 0 and ws(1 << 31, 10, 4) == 0
    for k in (0, 1, 100, 2048, 2049, 1 << 20):
        for e in (0, 511, 512, 513, 10_000, 30_000_000):
            for d in (1, 3, 50, 256):
                b = ws(k, e, d)
                assert b > 0 and b % 256 == 0, (k, e, d, b)
                assert ws(k + 1, e, d) >= b and ws(k, e + 1, d) >= b and ws(k, e, d + 1) >= b, (k, e, d)
    assert native.CSR_MEAN_CHUNK == 512
    # the partial sums: one [dim] row per chunk of a row longer than the chunk
    assert ws(1, 100 * 512, 256) - ws(1, 0, 256) >= 100 * 256 * 4
    assert ws(1, 513, 256) >= 2 * 256 * 4
    assert ops.csr_sum_workspace_bytes(1, 100 * 512, 256) == ws(1, 100 * 512, 256)


def test_group_rows_is_a_stable_grouping_on_cpu_tensors():
    rng = np.random.default_rng(0)
    k, n = 40, 3000
    index = rng.integers(0, k, n)
    index[index % 7 == 3] = 5                                      # groups 3, 10, 17, ... are empty, group 5 is large
    for dtype in (torch.int32, torch.int64):
        rp, col = ops.group_rows(torch.from_numpy(index).to(dtype), k)
        assert rp.dtype == torch.int64 and col.dtype == torch.int32 and rp.shape == (k + 1,) and col.shape == (n,)
        rp, col = rp.numpy(), col.numpy()
        assert rp[0] == 0 and rp[-1] == n and np.all(np.diff(rp) >= 0)
        assert np.array_equal(np.diff(rp), np.bincount(index, minlength=k))
        assert np.array_equal(np.sort(col), np.arange(n))         # every position once
        for g in range(k):
            members = col[rp[g]:rp[g + 1]]
            assert np.all(index[members] == g)
            assert np.all(np.diff(members) > 0), "positions inside a group must ascend (stable sort)"
        for g in (3, 10, 17):
            assert rp[g] == rp[g + 1]                             # an empty group: equal consecutive pointers
    rp, col = ops.group_rows(torch.zeros(0, dtype=torch.int32), 4)
    assert rp.tolist() == [0, 0, 0, 0, 0] and col.numel() == 0
    rp, col = ops.group_rows(torch.zeros(9, dtype=torch.int32), 1)  # one group of everything
    assert rp.tolist() == [0, 9] and col.tolist() == list(range(9))


def test_group_rows_refuses_an_index_outside_the_groups():
    for bad in (-1, 6, 1 << 20):
        idx = torch.tensor([0, 5, 2, bad, 1], dtype=torch.int32)
        with pytest.raises(native.SageError):
            ops.group_rows(idx, 6)
    with pytest.raises(native.SageError):
        ops.group_rows(torch.zeros(3), 4)                          # not an integer index


def test_embedding_entry_points_import_without_gpu():
    from sage355 import autograd, fullgraph
    assert callable(autograd.embed_rows) and callable(ops.csr_sum) and callable(fullgraph.one_hot_index) and callable(fullgraph.degree_index)
    idx, k = fullgraph.degree_index(torch.tensor([0, 2, 2, 7, 8]))
    assert idx.dtype == torch.int32 and idx.tolist() == [2, 0, 5, 1] and k == 6
    idx, k = fullgraph.one_hot_index(5, device="cpu")
    assert idx.tolist() == [0, 1, 2, 3, 4] and k == 5
    w = torch.randn(6, 3)
    assert torch.equal(autograd.embed_rows(w, torch.tensor([5, 0, 5], dtype=torch.int32)), w[[5, 0, 5]])   # no grad: plain index_select
