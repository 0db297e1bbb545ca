"""CPU checks of the sampled path's embedding gradient (sage_embed_grad): the symbols, argument validation before any launch, the
workspace query as host arithmetic, and the refusals of an indexed TwoHopEngine / EngineTrainer that need no device."""
import ctypes
import os
import re

import pytest
import torch

from sage355 import native, ops
from sage355.engine import TwoHopEngine
from sage355.train import EngineTrainer, run_engine_training

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_embed_grad_is_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in ("sage_embed_grad", "sage_embed_grad_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
    assert L.sage_embed_grad_workspace_bytes.restype is ctypes.c_size_t
    assert L.sage_embed_grad.restype is ctypes.c_int32
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9
    assert callable(ops.embed_grad) and callable(ops.embed_grad_workspace_bytes) and callable(ops.row_order)


def test_embed_grad_rejects_bad_arguments_before_any_launch():
    L = native.lib()
    args = dict(ldg=8, dim=8, k=5, n=100, embed_rows=7, ld=8)

    def call(**kw):                                               # every array NULL: whatever else is wrong, nothing can be launched
        a = dict(args, **kw)
        return L.sage_embed_grad(None, a["ldg"], a["dim"], None, None, a["k"], a["n"], None, None, None, a["embed_rows"], a["ld"], None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(dim=0), b"dim"), (dict(dim=6), b"dim"), (dict(dim=-4), b"dim"), (dict(ldg=4), b"ldg"), (dict(ldg=10), b"ldg"),
                     (dict(ld=4), b"ld ="), (dict(ld=9), b"ld ="), (dict(n=-1), b"n ="), (dict(k=0), b"k ="), (dict(n=1 << 20, k=1 << 11), b"n * k"),
                     (dict(embed_rows=0), b"embed_rows"), (dict(embed_rows=1 << 31), b"embed_rows")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())


def test_embed_grad_alignment_and_workspace_are_checked_before_any_launch():
    """Arrays that are not NULL (host memory: nothing may be launched on them): a misaligned gradient array, then a short, a missing
    and a misaligned workspace; with n == 0 the call returns SAGE_OK without a launch, workspace or not."""
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()
    base_arr = (ctypes.addressof(arr) + 15) // 16 * 16
    p = ctypes.c_void_p(base_arr)
    need = L.sage_embed_grad_workspace_bytes(100, 5, 7, 8)
    assert need > 0
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    def call(ws, nbytes, n=100, g=p, out=p):
        return L.sage_embed_grad(g, 8, 8, p, p, 5, n, None, None, out, 7, 8, ctypes.c_void_p(ws) if ws is not None else None, nbytes, None)

    assert call(base, need, g=ctypes.c_void_p(base_arr + 4)) == native.EINVAL and b"aligned" in L.sage_last_error()
    assert call(base, need, out=ctypes.c_void_p(base_arr + 8)) == native.EINVAL and b"aligned" in L.sage_last_error()
    assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert call(base, 0) == native.ENOSPACE
    assert call(None, need) == native.ENOSPACE
    assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
    assert call(base, need, n=0) == 0
    assert call(None, 0, n=0) == 0


def test_embed_grad_workspace_query_is_host_arithmetic():
    ws = native.lib().sage_embed_grad_workspace_bytes
    assert ws(-1, 5, 7, 8) == 0 and ws(10, 0, 7, 8) == 0 and ws(10, 5, 0, 8) == 0 and ws(10, 5, 1 << 31, 8) == 0 and ws(10, 5, 7, 0) == 0
    assert ws(1 << 20, 1 << 11, 7, 8) == 0                                   # n * k >= 2^31
    assert native.CSR_MEAN_CHUNK == 512
    for n in (1, 100, 1025, 30_000, 120_000):
        for k in (1, 7, 25, 64):
            for rows in (1, 13, 2048, 2049, 1 << 20):
                for d in (4, 52, 256):
                    b = ws(n, k, rows, d)
                    assert b > 0 and b % 256 == 0, (n, k, rows, d, b)
                    assert ws(n + 1, k, rows, d) >= b and ws(n, k + 1, rows, d) >= b and ws(n, k, rows, d + 4) >= b, (n, k, rows, d)
                    # the partial sums: one [dim] row per chunk of every run longer than a chunk
                    partial_rows = n * k // 512 + min(rows, n * k // 513)
                    assert b >= partial_rows * d * 4 + 4 * n * k * 4, (n, k, rows, d, b, partial_rows)
    assert ws(1, 513, 1, 256) >= 2 * 256 * 4
    assert ops.embed_grad_workspace_bytes(30_000, 25, 300, 256) == ws(30_000, 25, 300, 256)


def _tiny():
    rowptr = torch.tensor([0, 2, 3, 3, 5, 6, 6, 7, 8, 8, 9], dtype=torch.int64)
    col = torch.tensor([1, 3, 0, 0, 4, 3, 7, 6, 0], dtype=torch.int32)
    index = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2, 0], dtype=torch.int32)
    return rowptr, col, index


@pytest.mark.parametrize("kw,word", [(dict(concat=True), "concat"), (dict(agg_self_loop=True), "self loop"), (dict(relabel="degree"), "relabel"),
                                     (dict(slice_major=True), "slice-major")])
def test_an_indexed_engine_refuses_the_forms_it_does_not_provide(kw, word):
    rowptr, col, index = _tiny()
    m = 2 if kw.get("concat") else 1
    with pytest.raises(native.SageError, match=word):
        TwoHopEngine(rowptr, col, torch.zeros(3, 8), torch.zeros(4, m * 8), torch.zeros(4, m * 4), 2, 2, embed_index=index, **kw)


def test_an_indexed_engine_checks_its_embedding_and_its_index_once_at_construction():
    rowptr, col, index = _tiny()
    w1, w2 = torch.zeros(4, 8), torch.zeros(4, 4)
    bad = index.clone()
    bad[4] = 3
    low = index.clone()
    low[0] = -1
    for table, idx, word in [(torch.zeros(3, 6), index, "multiple of 4"), (torch.zeros(11, 8), index, "R = 11"), (torch.zeros(3, 8), bad, "value 3"),
                             (torch.zeros(3, 8), low, "value -1"), (torch.zeros(3, 8), index[:9], "int32 tensor"),
                             (torch.zeros(3, 8), index.long(), "int32 tensor")]:
        with pytest.raises(native.SageError, match=word):
            TwoHopEngine(rowptr, col, table, w1, w2, 2, 2, embed_index=idx)


def test_an_embedding_trainer_refuses_what_it_does_not_provide():
    rowptr, col, index = _tiny()
    kw = dict(embed_index=index, embed_rows=3, embed_dim=8)
    with pytest.raises(native.SageError, match="alternatives"):
        EngineTrainer(rowptr, col, torch.zeros(10, 8), 3, **kw)
    with pytest.raises(native.SageError, match="embed_rows"):
        EngineTrainer(rowptr, col, None, 3, embed_index=index, embed_dim=8)
    with pytest.raises(native.SageError, match="embed_dim"):
        EngineTrainer(rowptr, col, None, 3, embed_index=index, embed_rows=3)
    with pytest.raises(native.SageError, match="act1"):
        EngineTrainer(rowptr, col, None, 3, act1=7, **kw)
    for extra, word in [(dict(gcn=False), "concat"), (dict(agg_self_loop=True), "self loop"), (dict(relabel="degree"), "relabel")]:
        with pytest.raises(native.SageError, match=word):
            EngineTrainer(rowptr, col, None, 3, **kw, **extra)
    with pytest.raises(native.SageError, match="multiple of 4"):
        EngineTrainer(rowptr, col, None, 3, embed_index=index, embed_rows=3, embed_dim=6)
    with pytest.raises(native.SageError, match="R = 11"):
        EngineTrainer(rowptr, col, None, 3, embed_index=index, embed_rows=11, embed_dim=8)
    with pytest.raises(native.SageError, match="initializer"):
        run_engine_training(None, None, None, 3, initializer="pagerank")
