"""CPU checks of the touched-rows embedding gradient and sparse SGD update (sage_embed_grad_rows): the symbols, argument validation
before any launch, the workspace query as host arithmetic that does not grow with embed_rows, and the refusals of EngineTrainer /
TwoHopEngine that need no device."""
import ctypes
import os
import re

import pytest
import torch

from sage355 import native, ops
from sage355.engine import TwoHopEngine
from sage355.train import EngineTrainer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_embed_grad_rows_is_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in ("sage_embed_grad_rows", "sage_embed_grad_rows_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
    assert L.sage_embed_grad_rows_workspace_bytes.restype is ctypes.c_size_t
    assert L.sage_embed_grad_rows.restype is ctypes.c_int32
    assert len(L.sage_embed_grad_rows.argtypes) == 21
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9
    assert callable(ops.embed_grad_rows) and callable(ops.embed_grad_rows_workspace_bytes)


def _host_pointer():
    """A 16-byte aligned address inside host memory that stays alive with the returned array: nothing may be launched on it."""
    arr = (ctypes.c_int64 * 64)()
    return arr, (ctypes.addressof(arr) + 15) // 16 * 16


def test_embed_grad_rows_rejects_bad_arguments_before_any_launch():
    """sage_embed_grad's cases with every array NULL, then the cases of the new arguments with host memory where a pointer has to be
    present for the check to be reached."""
    L = native.lib()
    args = dict(ldg=8, dim=8, k=5, n=100, embed_rows=7, max_rows=7, ldr=8, lde=8, num=None, rows=None, grad=None, embed=None, g=None, nbr=None,
                cnt=None)

    def call(**kw):
        a = dict(args, **kw)
        return L.sage_embed_grad_rows(a["g"], a["ldg"], a["dim"], a["nbr"], a["cnt"], a["k"], a["n"], None, None, a["embed_rows"], a["num"],
                                      a["rows"], a["grad"], a["max_rows"], a["ldr"], a["embed"], a["lde"], 0.5, None, 0, None)

    assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
    for kw, word in [(dict(dim=0), b"dim"), (dict(dim=6), b"dim"), (dict(dim=-4), b"dim"), (dict(ldg=4), b"ldg"), (dict(ldg=10), b"ldg"),
                     (dict(n=-1), b"n ="), (dict(k=0), b"k ="), (dict(n=1 << 20, k=1 << 11), b"n * k"),
                     (dict(embed_rows=0), b"embed_rows"), (dict(embed_rows=1 << 31), b"embed_rows")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())
    arr, base = _host_pointer()
    p = ctypes.c_void_p(base)
    full = dict(g=p, nbr=p, cnt=p, num=p)
    # shapes of the optional arrays, checked where the array is given -- and before the pointers: the required ones are still NULL here
    for kw, word in [(dict(grad=p, rows=p, ldr=4), b"ldr"), (dict(grad=p, rows=p, ldr=10), b"ldr"), (dict(embed=p, lde=4), b"lde"),
                     (dict(embed=p, lde=9), b"lde"), (dict(grad=p, rows=p, max_rows=0), b"max_rows"), (dict(grad=p, rows=p, max_rows=-3), b"max_rows")]:
        assert call(**kw) == native.EINVAL, kw
        assert word in L.sage_last_error(), (kw, L.sage_last_error())
        assert call(**dict(full, **kw)) == native.EINVAL and word in L.sage_last_error(), kw
    assert call(g=p, nbr=p, cnt=p, grad=p, rows=p) == native.EINVAL and b"NULL" in L.sage_last_error()          # num_rows_out is required
    assert call(**full) == native.EINVAL and b"neither" in L.sage_last_error()
    assert call(**full, rows=p) == native.EINVAL and b"neither" in L.sage_last_error()
    assert call(**full, grad=p) == native.EINVAL and b"rows_out" in L.sage_last_error()
    assert call(**full, grad=p, embed=p) == native.EINVAL and b"rows_out" in L.sage_last_error()
    # everything in order but the workspace: that is the next thing looked at
    assert call(**full, embed=p) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert call(**full, grad=p, rows=p) == native.ENOSPACE
    del arr


def test_embed_grad_rows_alignment_and_workspace_are_checked_before_any_launch():
    """Arrays in host memory (nothing may be launched on them): a misaligned grad_agg, grad_rows and embed, then a short, a missing
    and a misaligned workspace; with n == 0 the call returns SAGE_OK without a launch, workspace or not."""
    L = native.lib()
    arr, base_arr = _host_pointer()
    p = ctypes.c_void_p(base_arr)
    need = L.sage_embed_grad_rows_workspace_bytes(100, 5, 7, 8)
    assert need > 0
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    def call(ws, nbytes, n=100, g=p, grad=p, embed=p):
        return L.sage_embed_grad_rows(g, 8, 8, p, p, 5, n, None, None, 7, p, p, grad, 7, 8, embed, 8, 0.5,
                                      ctypes.c_void_p(ws) if ws is not None else None, nbytes, None)

    for kw in (dict(g=ctypes.c_void_p(base_arr + 4)), dict(grad=ctypes.c_void_p(base_arr + 8)), dict(embed=ctypes.c_void_p(base_arr + 4)),
               dict(grad=None, embed=ctypes.c_void_p(base_arr + 8)), dict(embed=None, grad=ctypes.c_void_p(base_arr + 4))):
        assert call(base, need, **kw) == native.EINVAL and b"aligned" in L.sage_last_error(), kw
    for kw in (dict(), dict(grad=None), dict(embed=None)):
        assert call(base, need - 256, **kw) == native.ENOSPACE and b"workspace" in L.sage_last_error()
        assert call(base, 0, **kw) == native.ENOSPACE
        assert call(None, need, **kw) == native.ENOSPACE
        assert call(base + 4, need, **kw) == native.EINVAL and b"aligned" in L.sage_last_error()
        assert call(base, need, n=0, **kw) == 0
        assert call(None, 0, n=0, **kw) == 0
    del arr, buf


def test_embed_grad_rows_workspace_query_is_host_arithmetic_and_does_not_grow_with_embed_rows():
    ws = native.lib().sage_embed_grad_rows_workspace_bytes
    assert ws(-1, 5, 7, 8) == 0 and ws(10, 0, 7, 8) == 0 and ws(10, 5, 0, 8) == 0 and ws(10, 5, 1 << 31, 8) == 0 and ws(10, 5, 7, 0) == 0
    assert ws(1 << 20, 1 << 11, 7, 8) == 0                                   # n * k >= 2^31
    assert ws(0, 5, 7, 8) == 256
    for n in (1, 100, 1025, 30_000, 120_000):
        for k in (1, 7, 25, 64):
            for rows in (1, 13, 2048, 2049, 1 << 20, (1 << 31) - 1):
                for d in (4, 52, 256):
                    b = ws(n, k, rows, d)
                    assert b > 0 and b % 256 == 0, (n, k, rows, d, b)
                    assert ws(n + 1, k, rows, d) >= b and ws(n, k + 1, rows, d) >= b and ws(n, k, rows, d + 4) >= b, (n, k, rows, d)
                    # the partial sums (one [dim] row per chunk of every run longer than a chunk) and the four key / value arrays
                    partial_rows = n * k // 512 + min(rows, n * k // 513)
                    assert b >= partial_rows * d * 4 + 4 * n * k * 4, (n, k, rows, d, b, partial_rows)
                    # nothing sized by embed_rows: a bound in the slots alone -- 16 bytes of keys and values, 16 of sort temporary,
                    # 20 of run list and chunk offsets, the partial rows (at most 2 * slots / 512 + 1), 4 per set, and the padding
                    slots = n * k
                    assert b <= 56 * slots + (2 * slots // 512 + 1) * (d * 4 + 4) + 4 * n + 65536 + 16 * 256, (n, k, rows, d, b)
    for n, k in ((1, 1), (7, 100), (64, 1025)):
        for d in (4, 256):
            same = {ws(n, k, rows, d) for rows in (n * k, 1 << 20, (1 << 31) - 1) if rows >= n * k}
            assert len(same) == 1 and 0 not in same, (n, k, d, same)
    assert ops.embed_grad_rows_workspace_bytes(30_000, 25, 300, 256) == ws(30_000, 25, 300, 256)
    # the dense call's workspace holds three arrays of embed_rows entries; this one does not
    dense = native.lib().sage_embed_grad_workspace_bytes
    assert dense(4096, 15, 1 << 23, 256) - dense(4096, 15, 1 << 20, 256) >= 7 * (1 << 20) * 16
    assert ws(4096, 15, 1 << 23, 256) == ws(4096, 15, 1 << 20, 256)


def _tiny():
    rowptr = torch.tensor([0, 2, 3, 3, 5, 6, 6, 7, 8, 8, 9], dtype=torch.int64)
    col = torch.tensor([1, 3, 0, 0, 4, 3, 7, 6, 0], dtype=torch.int32)
    return rowptr, col


def test_a_sparse_trainer_needs_an_embedding():
    rowptr, col = _tiny()
    with pytest.raises(native.SageError, match="sparse_embed"):
        EngineTrainer(rowptr, col, torch.zeros(10, 8), 3, sparse_embed=True)
    assert EngineTrainer.__init__.__defaults__[-1] is False, "sparse_embed must default to False"


def test_the_compact_forms_are_refused_on_a_plain_engine_as_the_dense_one_is():
    """backward_weights looks at need_embed before it touches the device or any other field: an engine object without embed_index
    (no device needed to make one) is enough to reach every refusal."""
    eng = TwoHopEngine.__new__(TwoHopEngine)
    eng.embed_index = None
    for form, lr in ((True, None), ("rows", None), ("rows", 0.5), ("update", 0.5)):
        with pytest.raises(native.SageError, match="need_embed"):
            eng.backward_weights(None, None, need_embed=form, embed_lr=lr)
    eng.embed_index = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(native.SageError, match="embed_lr"):
        eng.backward_weights(None, None, need_embed="update")
    with pytest.raises(native.SageError, match="embed_lr"):
        eng.backward_weights(None, None, need_embed=True, embed_lr=0.5)
    with pytest.raises(native.SageError, match="need_embed"):
        eng.backward_weights(None, None, need_embed="dense")
