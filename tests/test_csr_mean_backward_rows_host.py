"""CPU checks of the seed-batch adjoint of the indexed mean (sage_csr_mean_backward_rows) and of its Python surface: the symbols,
every refusal before any launch (shapes, then NULL arrays one at a time, then the workspace), the size query as host arithmetic."""
import ctypes
import importlib
import inspect
import os
import re

import pytest

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = native.CSR_MEAN_CHUNK
NEW = ("sage_csr_mean_backward_rows_workspace_bytes", "sage_csr_mean_backward_rows")


def test_the_new_entries_are_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert len(L.sage_csr_mean_backward_rows.argtypes) == 18 and len(L.sage_csr_mean_backward_rows_workspace_bytes.argtypes) == 4
    assert L.sage_csr_mean_backward_rows_workspace_bytes.restype is ctypes.c_size_t
    assert L.sage_csr_mean_backward_rows.restype is ctypes.c_int32
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9
    mk = open(os.path.join(REPO, "graphsage-simple_amd", "csrc", "Makefile")).read()
    assert "sage_csr_mean_backward_rows.hip" in mk


def _call(L, arrays, ws=None, nbytes=0, **kw):
    """arrays: (rowptr, col, nodes, index, grad_out, grad_table, total_terms)"""
    a = dict(dict(num_nodes=10, n=5, max_edges=100, num_rows=7, ldg=4, dim=4, self_loop=0, ldgt=4), **kw)
    rowptr, col, nodes, index, grad_out, grad_table, total = arrays
    return L.sage_csr_mean_backward_rows(rowptr, col, a["num_nodes"], nodes, a["n"], a["max_edges"], index, a["num_rows"], grad_out, a["ldg"],
                                         a["dim"], a["self_loop"], grad_table, a["ldgt"], total, ws, nbytes, None)


def test_bad_shapes_are_refused_first_whatever_the_pointers_are():
    L = native.lib()
    none = (None,) * 7                                            # every array NULL: whatever else is wrong, nothing can be launched
    assert _call(L, none) == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(num_nodes=-1), b"num_nodes"), (dict(num_nodes=1 << 31), b"num_nodes"), (dict(n=-1), b"n ="),
                     (dict(max_edges=-1), b"max_edges"), (dict(num_rows=-1), b"num_rows"), (dict(num_rows=(1 << 31) - 1), b"num_rows"),
                     (dict(num_rows=0), b"num_rows = 0"), (dict(dim=0), b"dim"), (dict(ldg=3), b"ldg"), (dict(ldgt=2), b"ldgt"),
                     (dict(self_loop=2), b"self_loop"), (dict(self_loop=-1), b"self_loop")]:
        assert _call(L, none, **kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())


def test_null_arrays_are_refused_one_at_a_time_and_the_nullable_ones_are_not():
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()                                 # host memory: nothing may be launched on it
    p = ctypes.cast(arr, ctypes.c_void_p)
    for missing in (0, 1, 2, 4, 5):                               # rowptr, col, nodes, grad_out, grad_table
        a = [None if i == missing else p for i in range(7)]
        assert _call(L, a) == native.EINVAL and b"NULL" in L.sage_last_error(), missing
    for missing in (3, 6):                                        # index and total_terms may be NULL: the next refusal is the workspace's
        a = [None if i == missing else p for i in range(7)]
        assert _call(L, a) == native.ENOSPACE and b"workspace" in L.sage_last_error(), missing
    # term positions past an int32: refused as a shape out of range, after the arrays
    assert _call(L, (p,) * 7, max_edges=(1 << 31) - 5) == native.EINVAL and b"out of range" in L.sage_last_error()


def test_the_workspace_is_checked_before_any_launch():
    """Arrays that are not NULL (host memory), then a short, a missing and a misaligned workspace; with no table rows and a good
    workspace the call returns SAGE_OK without a launch."""
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    need = L.sage_csr_mean_backward_rows_workspace_bytes(5, 100, 7, 4)
    assert need > 0
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    full = (p,) * 7
    assert _call(L, full, ctypes.c_void_p(base), need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert _call(L, full, ctypes.c_void_p(base), 0) == native.ENOSPACE
    assert _call(L, full, None, need) == native.ENOSPACE
    assert _call(L, full, ctypes.c_void_p(base + 4), need) == native.EINVAL and b"aligned" in L.sage_last_error()
    need0 = L.sage_csr_mean_backward_rows_workspace_bytes(0, 100, 0, 4)
    assert 0 < need0 <= need
    assert _call(L, full, ctypes.c_void_p(base), need0, n=0, num_rows=0) == 0          # no rows: SAGE_OK without a launch
    assert _call(L, full, ctypes.c_void_p(base), need, num_rows=0) == native.EINVAL    # ... but not with seed rows


def test_the_workspace_query_is_host_arithmetic():
    ws = native.lib().sage_csr_mean_backward_rows_workspace_bytes
    assert ws(-1, 10, 10, 4) == 0 and ws(10, -1, 10, 4) == 0 and ws(10, 10, -1, 4) == 0 and ws(10, 10, 10, 0) == 0
    assert ws(10, 10, (1 << 31) - 1, 4) == 0                      # num_rows is a sort key with a sentinel above it
    assert ws(10, (1 << 31) - 10, 10, 4) == 0 and ws(10, 1 << 50, 10, 4) == 0          # max_edges + n term positions: below 2^31
    for n in (0, 1, 100, 2049, 4096):
        for e in (0, 1, E, E + 1, 10_000, 30_000_000):
            for rows in (0, 1, 4096, 1 << 20):
                for d in (1, 3, 128):
                    b = ws(n, e, rows, d)
                    assert b > 0 and b % 256 == 0, (n, e, rows, d, b)
                    assert ws(n + 1, e, rows, d) >= b and ws(n, e + 1, rows, d) >= b and ws(n, e, rows + 1, d) >= b and ws(n, e, rows, d + 1) >= b
                    assert ws(n, e + 128 * E, rows, d) > b, (n, e, rows, d)              # monotone in max_edges, strictly over many chunks
    # a term position costs its key and value, twice (the sort's two sides), and the sort's temporary
    assert ws(10, 1 << 20, 10, 4) - ws(10, 0, 10, 4) >= (1 << 20) * 16
    # nothing is sized by the graph: the query does not even take num_nodes
    assert ops.csr_mean_backward_rows_workspace_bytes(4096, 1 << 20, 70_000, 128) == ws(4096, 1 << 20, 70_000, 128)


def test_the_python_surface_has_the_documented_signatures():
    import torch

    from sage355 import autograd
    exactbatch = importlib.import_module("sage355.exactbatch")
    assert list(inspect.signature(ops.csr_mean_backward_rows).parameters) == [
        "rowptr", "col", "nodes", "grad_out", "index", "num_rows", "self_loop", "out", "max_edges", "workspace", "total_terms"]
    assert list(inspect.signature(ops.csr_mean_backward_rows_workspace_bytes).parameters) == ["n", "max_edges", "num_rows", "dim"]
    sig = inspect.signature(autograd.csr_mean_rows)
    assert list(sig.parameters) == ["rowptr", "col", "table", "nodes", "index", "self_loop", "any_nonempty", "max_edges"]
    assert sig.parameters["index"].default is None and sig.parameters["self_loop"].default is False
    sig = inspect.signature(exactbatch.ExactBatchTrainer.__init__)
    assert list(sig.parameters) == ["self", "rowptr", "col", "table", "num_classes", "hidden1", "hidden2", "gcn", "lr", "agg_self_loop", "head",
                                    "rowptr_outer", "col_outer", "act1"]
    assert (sig.parameters["hidden1"].default, sig.parameters["hidden2"].default, sig.parameters["lr"].default) == (50, 128, 0.7)
    assert sig.parameters["head"].default == "native" and sig.parameters["act1"].default == native.ACT_RELU
    for name in ("parameters", "grads", "step", "predict", "forward"):
        assert callable(getattr(exactbatch.ExactBatchTrainer, name))
    sig = inspect.signature(exactbatch.run_exact_batch_training)
    assert list(sig.parameters)[:7] == ["graph", "feat_data", "labels", "num_classes", "seed", "epochs", "batch_size"]
    assert (sig.parameters["seed"].default, sig.parameters["epochs"].default, sig.parameters["batch_size"].default) == (1, 1, 128)
    if not torch.cuda.is_available():
        rp = torch.tensor([0, 1, 2])
        col = torch.tensor([1, 0], dtype=torch.int32)
        with pytest.raises(native.SageError):
            ops.csr_mean_backward_rows(rp, col, torch.tensor([0], dtype=torch.int32), torch.zeros(1, 4))
        with pytest.raises(native.SageError):
            exactbatch.ExactBatchTrainer(rp, col, torch.zeros(2, 4), 3)
