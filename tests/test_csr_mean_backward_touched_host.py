"""CPU checks of the touched-rows form of the seed-batch adjoint (sage_csr_mean_backward_touched) and of its Python surface: the
symbols, every refusal before any launch (shapes, then NULL arrays one at a time, then the workspace), the size query as host
arithmetic that does not grow with num_rows, and the refusals of ExactBatchEmbedTrainer / run_exact_batch_training that need no GPU."""
import ctypes
import importlib
import inspect
import os
import re

import pytest

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = native.CSR_MEAN_CHUNK
NEW = ("sage_csr_mean_backward_touched_workspace_bytes", "sage_csr_mean_backward_touched")
# the arrays of a call, in argument order; the nullable ones: index, total_terms, and one of (rows_out + grad_rows) / table
ARRAYS = ("rowptr", "col", "nodes", "index", "grad_out", "num_rows_out", "rows_out", "grad_rows", "table", "total_terms")


def test_the_new_entries_are_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert len(L.sage_csr_mean_backward_touched.argtypes) == 24 and len(L.sage_csr_mean_backward_touched_workspace_bytes.argtypes) == 4
    assert L.sage_csr_mean_backward_touched.argtypes[19] is ctypes.c_float          # lr
    assert L.sage_csr_mean_backward_touched_workspace_bytes.restype is ctypes.c_size_t
    assert L.sage_csr_mean_backward_touched.restype is ctypes.c_int32
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9


def _call(L, arrays, ws=None, nbytes=0, **kw):
    a = dict(dict(num_nodes=10, n=5, max_edges=100, num_rows=7, ldg=4, dim=4, self_loop=0, max_rows=7, ldr=4, ldt=4, lr=0.5), **kw)
    p = dict(zip(ARRAYS, arrays))
    return L.sage_csr_mean_backward_touched(p["rowptr"], p["col"], a["num_nodes"], p["nodes"], a["n"], a["max_edges"], p["index"], a["num_rows"],
                                            p["grad_out"], a["ldg"], a["dim"], a["self_loop"], p["num_rows_out"], p["rows_out"], p["grad_rows"],
                                            a["max_rows"], a["ldr"], p["table"], a["ldt"], a["lr"], p["total_terms"], ws, nbytes, None)


def _host_pointer():
    arr = (ctypes.c_int64 * 64)()                                 # host memory: nothing may be launched on it
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_bad_shapes_are_refused_first_whatever_the_pointers_are():
    L = native.lib()
    none = (None,) * len(ARRAYS)                                  # every array NULL: whatever else is wrong, nothing can be launched
    assert _call(L, none) == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(num_nodes=-1), b"num_nodes"), (dict(num_nodes=1 << 31), b"num_nodes"), (dict(n=-1), b"n ="),
                     (dict(max_edges=-1), b"max_edges"), (dict(num_rows=-1), b"num_rows"), (dict(num_rows=(1 << 31) - 1), b"num_rows"),
                     (dict(num_rows=0), b"num_rows = 0"), (dict(dim=0), b"dim"), (dict(ldg=3), b"ldg"),
                     (dict(self_loop=2), b"self_loop"), (dict(self_loop=-1), b"self_loop")]:
        assert _call(L, none, **kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())
    # the leading dimension and the capacity of an output count only where that output is given
    keep, p = _host_pointer()
    with_grad = [p if name == "grad_rows" else None for name in ARRAYS]
    with_table = [p if name == "table" else None for name in ARRAYS]
    for arrays, kw, word in [(with_grad, dict(ldr=3), b"ldr"), (with_grad, dict(max_rows=0), b"max_rows"), (with_table, dict(ldt=2), b"ldt")]:
        assert _call(L, arrays, **kw) == native.EINVAL and word in L.sage_last_error(), (kw, L.sage_last_error())
    for kw in (dict(ldr=0, max_rows=0), dict(ldt=0)):             # ... and not where it is NULL: the next refusal is the arrays'
        assert _call(L, none, **kw) == native.EINVAL and b"NULL" in L.sage_last_error(), kw


def test_null_arrays_are_refused_one_at_a_time_and_the_nullable_ones_are_not():
    L = native.lib()
    keep, p = _host_pointer()
    for missing in ("rowptr", "col", "nodes", "grad_out", "num_rows_out"):
        a = [None if name == missing else p for name in ARRAYS]
        assert _call(L, a) == native.EINVAL and b"NULL" in L.sage_last_error(), missing
    # index and total_terms may be NULL, and so may the gradient pair or the table: the next refusal is the workspace's
    for missing in (("index",), ("total_terms",), ("table",), ("rows_out", "grad_rows"), ("index", "total_terms", "table")):
        a = [None if name in missing else p for name in ARRAYS]
        assert _call(L, a) == native.ENOSPACE and b"workspace" in L.sage_last_error(), missing
    # neither output requested, and a gradient without its row list
    a = [None if name in ("rows_out", "grad_rows", "table") else p for name in ARRAYS]
    assert _call(L, a) == native.EINVAL and b"neither" in L.sage_last_error()
    a = [None if name == "rows_out" else p for name in ARRAYS]
    assert _call(L, a) == native.EINVAL and b"rows_out" in L.sage_last_error()
    # term positions past an int32: refused as a shape out of range, after the arrays
    assert _call(L, (p,) * len(ARRAYS), max_edges=(1 << 31) - 5) == native.EINVAL and b"out of range" in L.sage_last_error()


def test_the_workspace_is_checked_before_any_launch():
    """Arrays that are not NULL (host memory), then a short, a missing and a misaligned workspace; without seed rows and with a good
    workspace the call returns SAGE_OK without a launch."""
    L = native.lib()
    keep, p = _host_pointer()
    need = L.sage_csr_mean_backward_touched_workspace_bytes(5, 100, 7, 4)
    assert need > 0
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    full = (p,) * len(ARRAYS)
    assert _call(L, full, ctypes.c_void_p(base), need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert _call(L, full, ctypes.c_void_p(base), 0) == native.ENOSPACE
    assert _call(L, full, None, need) == native.ENOSPACE
    assert _call(L, full, ctypes.c_void_p(base + 4), need) == native.EINVAL and b"aligned" in L.sage_last_error()
    need0 = L.sage_csr_mean_backward_touched_workspace_bytes(0, 100, 7, 4)
    assert 0 < need0 <= need
    before = list(keep)
    assert _call(L, full, ctypes.c_void_p(base), need0, n=0) == 0                      # no seed rows: SAGE_OK without a launch
    assert _call(L, full, ctypes.c_void_p(base), need0, n=0, num_rows=0) == 0
    assert list(keep) == before
    assert _call(L, full, ctypes.c_void_p(base), need, num_rows=0) == native.EINVAL    # ... but no table rows with seed rows is refused


def test_the_workspace_query_is_host_arithmetic_and_does_not_grow_with_the_table():
    ws = native.lib().sage_csr_mean_backward_touched_workspace_bytes
    assert ws(-1, 10, 10, 4) == 0 and ws(10, -1, 10, 4) == 0 and ws(10, 10, -1, 4) == 0 and ws(10, 10, 10, 0) == 0
    assert ws(10, 10, (1 << 31) - 1, 4) == 0                      # num_rows is a sort key with a sentinel above it
    assert ws(10, (1 << 31) - 10, 10, 4) == 0 and ws(10, 1 << 50, 10, 4) == 0          # max_edges + n term positions: below 2^31
    for n in (0, 1, 100, 2049, 4096):
        for e in (0, 1, E, E + 1, 10_000, 30_000_000):
            for rows in (0, 1, 4096, 1 << 20):
                for d in (1, 3, 128):
                    b = ws(n, e, rows, d)
                    assert b > 0 and b % 256 == 0, (n, e, rows, d, b)
                    assert ws(n + 1, e, rows, d) >= b and ws(n, e + 1, rows, d) >= b and ws(n, e, rows, d + 1) >= b
                    assert ws(n, e + 128 * E, rows, d) > b, (n, e, rows, d)              # monotone in max_edges, strictly over many chunks
            # nothing is sized by the table once it has a row for every term position
            if n + e <= 1 << 20:
                for d in (1, 128):
                    assert ws(n, e, n + e, d) == ws(n, e, 1 << 20, d) == ws(n, e, (1 << 31) - 2, d), (n, e, d)
    # ... where the dense form pays for every table row
    dense = native.lib().sage_csr_mean_backward_rows_workspace_bytes
    assert dense(64, 1000, 1 << 24, 64) - dense(64, 1000, 2000, 64) >= (1 << 24) * 8
    assert ws(64, 1000, 1 << 24, 64) == ws(64, 1000, 2000, 64) < dense(64, 1000, 2000, 64) + 65536
    # a term position costs its key and value, twice (the sort's two sides), and the sort's temporary
    assert ws(10, 1 << 20, 10, 4) - ws(10, 0, 10, 4) >= (1 << 20) * 16
    assert ops.csr_mean_backward_touched_workspace_bytes(4096, 1 << 20, 70_000, 128) == ws(4096, 1 << 20, 70_000, 128)


def test_the_python_surface_has_the_documented_signatures():
    import torch

    exactbatch = importlib.import_module("sage355.exactbatch")
    assert list(inspect.signature(ops.csr_mean_backward_touched).parameters) == [
        "rowptr", "col", "nodes", "grad_out", "index", "num_rows", "self_loop", "max_edges", "max_rows", "table", "lr", "want_grad", "out",
        "workspace", "total_terms"]
    assert inspect.signature(ops.csr_mean_backward_touched).parameters["want_grad"].default is True
    assert list(inspect.signature(ops.csr_mean_backward_touched_workspace_bytes).parameters) == ["n", "max_edges", "num_rows", "dim"]
    assert issubclass(exactbatch.ExactBatchEmbedTrainer, exactbatch.ExactBatchTrainer)
    sig = inspect.signature(exactbatch.ExactBatchEmbedTrainer.__init__)
    assert list(sig.parameters) == ["self", "rowptr", "col", "num_classes", "embed_index", "embed_rows", "embed_dim", "hidden1", "hidden2", "gcn",
                                    "lr", "agg_self_loop", "head", "rowptr_outer", "col_outer", "act1", "sparse_embed"]
    assert (sig.parameters["hidden1"].default, sig.parameters["hidden2"].default, sig.parameters["lr"].default) == (50, 128, 0.7)
    assert sig.parameters["head"].default == "native" and sig.parameters["act1"].default == native.ACT_RELU
    assert sig.parameters["sparse_embed"].default is False and sig.parameters["gcn"].default is True
    sig = inspect.signature(exactbatch.run_exact_batch_training)
    assert list(sig.parameters)[:7] == ["graph", "feat_data", "labels", "num_classes", "seed", "epochs", "batch_size"]
    assert list(sig.parameters)[-3:] == ["initializer", "embed_dim", "sparse_embed"]
    assert (sig.parameters["initializer"].default, sig.parameters["embed_dim"].default, sig.parameters["sparse_embed"].default) == ("None", 100, False)
    if not torch.cuda.is_available():
        rp = torch.tensor([0, 1, 2])
        col = torch.tensor([1, 0], dtype=torch.int32)
        with pytest.raises(native.SageError):
            ops.csr_mean_backward_touched(rp, col, torch.tensor([0], dtype=torch.int32), torch.zeros(1, 4))


def test_the_trainer_and_the_driver_refuse_before_any_gpu_use():
    """Host tensors throughout: every one of these is refused before the trainer asks for a device."""
    import torch

    from sage355.exactbatch import ExactBatchEmbedTrainer, run_exact_batch_training
    rp = torch.tensor([0, 1, 2])
    col = torch.tensor([1, 0], dtype=torch.int32)
    index = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(native.SageError, match="embed_rows"):
        ExactBatchEmbedTrainer(rp, col, 3, index, None, 8)
    with pytest.raises(native.SageError, match="embed_rows"):
        ExactBatchEmbedTrainer(rp, col, 3, index, 0, 8)
    with pytest.raises(native.SageError, match="embed_dim"):
        ExactBatchEmbedTrainer(rp, col, 3, index, 2, None)
    with pytest.raises(native.SageError, match="embed_index"):
        ExactBatchEmbedTrainer(rp, col, 3, None, 2, 8)
    with pytest.raises(native.SageError, match="act1"):
        ExactBatchEmbedTrainer(rp, col, 3, index, 2, 8, act1=native.ACT_NONE)
    with pytest.raises(native.SageError, match="head"):
        ExactBatchEmbedTrainer(rp, col, 3, index, 2, 8, head="numpy")
    with pytest.raises(native.SageError, match="concat"):
        ExactBatchEmbedTrainer(rp, col, 3, index, 2, 8, gcn=False, sparse_embed=True)
    with pytest.raises(native.SageError, match="initializer"):
        run_exact_batch_training(None, None, None, 3, initializer="pagerank")
    with pytest.raises(native.SageError, match="sparse_embed"):
        run_exact_batch_training(None, None, None, 3, sparse_embed=True)
