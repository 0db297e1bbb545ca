"""CPU checks of the full-neighbourhood frontier (sage_csr_frontier, sage_csr_frontier_clear) and of embed_nodes' surface: the
symbols, every refusal before any launch, the workspace query as host arithmetic."""
import ctypes
import inspect
import os
import re

import pytest

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = native.CSR_MEAN_CHUNK
NEW = ("sage_csr_frontier_workspace_bytes", "sage_csr_frontier", "sage_csr_frontier_clear")


def test_the_new_entries_are_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert L.sage_csr_frontier_workspace_bytes.restype is ctypes.c_size_t
    assert L.sage_csr_frontier.restype is ctypes.c_int32 and L.sage_csr_frontier_clear.restype is ctypes.c_int32
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9


def test_csr_frontier_rejects_bad_arguments_before_any_launch():
    """Shapes first -- with every array NULL a bad shape is still reported as such -- then the NULL arrays, one at a time."""
    L = native.lib()
    args = dict(num_nodes=10, n=4, max_edges=100, max_nodes=10)

    def call(**kw):                                               # every array NULL: whatever else is wrong, nothing can be launched
        a = dict(args, **kw)
        return L.sage_csr_frontier(None, None, a["num_nodes"], None, a["n"], a["max_edges"], None, None, a["max_nodes"], None, None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(num_nodes=-1), b"num_nodes"), (dict(num_nodes=1 << 31), b"num_nodes"), (dict(n=-1), b"n ="),
                     (dict(max_nodes=-1), b"max_nodes"), (dict(max_edges=-1), b"max_edges")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())
    arr = (ctypes.c_int64 * 64)()                                 # host memory: nothing may be launched on it
    p = ctypes.cast(arr, ctypes.c_void_p)
    for missing in range(6):                                      # rowptr, col, seeds, pos, nodes_out, count
        a = [None if i == missing else p for i in range(6)]
        rc = L.sage_csr_frontier(a[0], a[1], 10, a[2], 4, 100, a[3], a[4], 10, a[5], None, 0, None)
        assert rc == native.EINVAL and b"NULL" in L.sage_last_error(), missing
    assert L.sage_csr_frontier_clear(None, None, None, 10, None) == native.EINVAL and b"NULL" in L.sage_last_error()
    for missing in range(3):
        a = [None if i == missing else p for i in range(3)]
        assert L.sage_csr_frontier_clear(a[0], a[1], a[2], 10, None) == native.EINVAL, missing
    assert L.sage_csr_frontier_clear(p, p, p, -1, None) == native.EINVAL and b"max_nodes" in L.sage_last_error()
    assert L.sage_csr_frontier_clear(None, None, None, -1, None) == native.EINVAL and b"max_nodes" in L.sage_last_error()
    assert L.sage_csr_frontier_clear(p, p, p, 0, None) == 0       # no rows: SAGE_OK without a launch


def test_the_workspace_is_checked_before_any_launch():
    """Arrays that are not NULL (host memory), then a short, a missing and a misaligned workspace; with no seeds and a good
    workspace the call returns SAGE_OK without a launch."""
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    need = L.sage_csr_frontier_workspace_bytes(10, 5000)
    assert need > 0
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    def call(ws, nbytes, n=10, max_edges=5000):
        return L.sage_csr_frontier(p, p, 10, p, n, max_edges, p, p, 10, p, ctypes.c_void_p(ws) if ws is not None else None, nbytes, None)

    assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert call(base, 0) == native.ENOSPACE
    assert call(None, need) == native.ENOSPACE
    assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
    assert call(base, need, max_edges=1 << 50) == native.EINVAL and b"out of range" in L.sage_last_error()
    assert call(base, L.sage_csr_frontier_workspace_bytes(0, 5000), n=0) == 0


def test_the_workspace_query_is_host_arithmetic():
    ws = native.lib().sage_csr_frontier_workspace_bytes
    assert ws(-1, 10) == 0 and ws(10, -1) == 0 and ws(10, 1 << 50) == 0
    for n in (0, 1, 100, 2049, 5000, 1 << 20):
        for e in (0, 1, E, E + 1, 30_000_000, 1 << 33):
            b = ws(n, e)
            assert b > 0 and b % 256 == 0, (n, e, b)
            assert ws(n + 1, e) >= b and ws(n, e + 1) >= b and ws(n + 4096, e) > b and ws(n, e + 128 * E) > b, (n, e)
    assert ws(10, 1000 * E) - ws(10, 0) >= 1000 * 4 - 256         # an item entry per chunk of a long row (an empty list is one 256-byte piece)
    assert ws(4096, 1 << 24) < 1 << 20                            # lists only: no partial sums, whatever the rows are wide
    assert ops.csr_frontier_workspace_bytes(4096, 1 << 24) == ws(4096, 1 << 24)


def test_the_python_surface_imports_and_refuses_without_a_gpu():
    import torch

    from sage355 import inference, train
    sig = inspect.signature(inference.embed_nodes)
    assert list(sig.parameters) == ["rowptr", "col", "table", "w1", "w2", "seeds", "concat", "agg_self_loop", "act1", "act2", "nan_empty",
                                    "rowptr_outer", "col_outer", "rows_per_call", "index", "frontier", "out"]
    assert sig.parameters["rows_per_call"].default == inference.ROWS_PER_CALL and sig.parameters["nan_empty"].default is True
    assert list(inspect.signature(inference.embed_nodes_from_modules).parameters)[:2] == ["enc2", "nodes"]
    assert list(inspect.signature(ops.csr_frontier).parameters) == ["rowptr", "col", "seeds", "frontier", "max_edges"]
    assert callable(train.EngineTrainer.embed_exact) and callable(train.EngineTrainer.predict_exact)
    assert inspect.signature(train.run_engine_training).parameters["exact_eval"].default is False
    if not torch.cuda.is_available():
        rp = torch.tensor([0, 1, 2])
        col = torch.tensor([1, 0], dtype=torch.int32)
        with pytest.raises(native.SageError):
            inference.embed_nodes(rp, col, torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(2, 3), [0, 1])
        with pytest.raises(native.SageError):
            ops.CsrFrontier(2, "cpu")
        with pytest.raises(native.SageError):
            ops.csr_frontier(rp, col, torch.tensor([0], dtype=torch.int32), None)
