"""CPU checks of the bf16-table full-neighbourhood mean (sage_csr_mean_bf16): the symbol, argument validation before any launch, the
workspace checks, the table_dtype parameters of the Python surface, and that bag-of-words stand-in features are exact in bf16."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_entry_is_declared_bound_and_exported_and_the_abi_is_still_9():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    assert re.search(r"\bsage_csr_mean_bf16\s*\(", text), "sage_csr_mean_bf16 is not declared in include/sage355.h"
    assert re.search(r"const\s+uint16_t\s*\*\s*table", text), "the bf16 table is declared as raw 16-bit values"
    assert "sage_csr_mean_bf16" in native.SYMBOLS and hasattr(L, "sage_csr_mean_bf16")
    assert L.sage_csr_mean_bf16.argtypes is not None and list(L.sage_csr_mean_bf16.argtypes) == list(L.sage_csr_mean.argtypes)
    assert L.sage_csr_mean_bf16.restype is ctypes.c_int32
    assert re.search(r"#define\s+SAGE_ABI_VERSION\s+9\b", text) and native.ABI_VERSION == 9 and L.sage_abi_version() == 9


def test_csr_mean_bf16_rejects_bad_arguments_before_any_launch():
    """sage_csr_mean's refusals in sage_csr_mean's order, under the entry's own name."""
    L = native.lib()
    args = dict(num_nodes=10, n=10, max_edges=100, table_rows=10, ld=4, dim=4, self_loop=0, ldo=4)

    def call(entry, **kw):                                        # every array NULL: whatever else is wrong, nothing can be launched
        a = dict(args, **kw)
        return entry(None, None, a["num_nodes"], None, a["n"], a["max_edges"], None, a["table_rows"], a["ld"], a["dim"], a["self_loop"],
                     None, None, a["ldo"], None, 0, None)

    assert call(L.sage_csr_mean_bf16) == native.EINVAL and b"NULL" in L.sage_last_error()
    assert L.sage_last_error().startswith(b"csr_mean_bf16:")
    cases = [(dict(dim=0), b"dim"), (dict(dim=-3), b"dim"), (dict(ld=3), b"ld ="), (dict(ldo=2), b"ldo"), (dict(num_nodes=-1), b"num_nodes"),
             (dict(num_nodes=1 << 31), b"num_nodes"), (dict(n=-1), b"n ="), (dict(n=11), b"without a node list"),
             (dict(max_edges=-1), b"max_edges"), (dict(table_rows=0), b"table_rows"), (dict(table_rows=1 << 31), b"table_rows"),
             (dict(self_loop=2), b"self_loop"),
             # two things wrong: the one sage_csr_mean names first is named
             (dict(num_nodes=-1, dim=0), b"num_nodes"), (dict(n=-1, max_edges=-1), b"n ="), (dict(max_edges=-1, dim=0), b"max_edges"),
             (dict(dim=0, table_rows=0), b"dim"), (dict(table_rows=0, self_loop=2), b"table_rows")]
    for kw, word in cases:
        assert call(L.sage_csr_mean_bf16, **kw) == native.EINVAL, kw
        msg = L.sage_last_error()
        assert word in msg and msg.startswith(b"csr_mean_bf16:"), (kw, msg)
        assert call(L.sage_csr_mean, **kw) == native.EINVAL                                    # the same refusal, the same words
        assert L.sage_last_error() == msg.replace(b"csr_mean_bf16:", b"csr_mean:", 1), (kw, msg, L.sage_last_error())


def test_the_workspace_is_checked_before_any_launch():
    """Arrays that are not NULL (host memory: nothing may be launched on them), then a short, a missing and a misaligned workspace;
    with no rows and a good workspace the call returns SAGE_OK without a launch.  The workspace is sage_csr_mean's: partials are fp32."""
    L = native.lib()
    arr = (ctypes.c_int64 * 64)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    need = L.sage_csr_mean_workspace_bytes(10, 5000, 4)
    assert need > 0
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    def call(ws, nbytes, n=10, max_edges=5000):
        return L.sage_csr_mean_bf16(p, p, 10, None, n, max_edges, p, 10, 4, 4, 1, None, p, 4, ctypes.c_void_p(ws), nbytes, None)

    assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error() and b"csr_mean_bf16" in L.sage_last_error()
    assert call(base, 0) == native.ENOSPACE
    assert call(None, need) == native.ENOSPACE
    assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
    assert call(base, need, max_edges=1 << 50) == native.EINVAL and b"out of range" in L.sage_last_error()
    assert call(base, L.sage_csr_mean_workspace_bytes(0, 5000, 4), n=0) == 0


def test_the_table_dtype_parameters_exist_with_fp32_defaults_and_import_without_gpu():
    from sage355 import exactbatch, fullgraph, inference
    for fn in (inference.embed_all_from_modules, inference.embed_nodes_from_modules, exactbatch.run_exact_batch_training,
               fullgraph.run_full_graph_training):
        assert inspect.signature(fn).parameters["table_dtype"].default is torch.float32, fn.__name__
    assert fullgraph.check_table_dtype("x", torch.bfloat16, False) is torch.bfloat16
    for dtype, embed in ((torch.float16, False), (torch.float64, False), (torch.bfloat16, True)):
        with pytest.raises(native.SageError):
            fullgraph.check_table_dtype("x", dtype, embed)
    t16 = torch.zeros(4, 4, dtype=torch.bfloat16)
    with pytest.raises(native.SageError, match="bfloat16"):
        ops.refuse_bf16(t16, "somebody")
    ops.refuse_bf16(t16.float(), "somebody")
    ops.refuse_bf16(None, "somebody")
    if not torch.cuda.is_available():
        rp = torch.tensor([0, 1, 2])
        col = torch.tensor([1, 0], dtype=torch.int32)
        with pytest.raises(native.SageError):
            ops.csr_mean(rp, col, torch.zeros(2, 4, dtype=torch.bfloat16))


def test_the_sampled_paths_refuse_a_bf16_table_by_name_before_any_gpu_use():
    """Host tensors throughout: the refusal names the dtype and comes before anything asks for a device."""
    from sage355.engine import RolePipeline, TwoHopEngine
    from sage355.fullgraph import FullGraphTrainer
    from sage355.train import EngineTrainer
    rp = torch.tensor([0, 1, 2])
    col = torch.tensor([1, 0], dtype=torch.int32)
    t16 = torch.zeros(2, 4, dtype=torch.bfloat16)
    w = torch.zeros(4, 4)
    idx = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(native.SageError, match="bfloat16"):
        TwoHopEngine(rp, col, t16, w, w, 2, 2)
    with pytest.raises(native.SageError, match="bfloat16"):
        RolePipeline(rp, col, t16, w, w, 2, 2, batch=2)
    with pytest.raises(native.SageError, match="bfloat16"):
        EngineTrainer(rp, col, t16, 3, hidden2=4, head="torch")
    with pytest.raises(native.SageError, match="bfloat16"):
        EngineTrainer(rp, col, t16, 3, hidden2=4, head="torch", embed_index=idx, embed_rows=2, embed_dim=4)
    with pytest.raises(native.SageError, match="bfloat16"):
        FullGraphTrainer(rp, col, t16, 3, hidden2=4, head="torch", embed_index=idx, embed_rows=2, embed_dim=4)


def test_standin_citation_features_are_exact_in_bf16():
    """Bag-of-words features are 0 and 1: storing them as bf16 rounds nothing."""
    from sage355.datasets import standin_citation
    from sage355.graph import rmat_graph
    graph = rmat_graph(11, 30_000, seed=4, accel=None)
    feats, _ = standin_citation(graph, num_classes=7, feat_dim=1433, seed=0)
    t = torch.as_tensor(np.asarray(feats), dtype=torch.float32)
    assert t.shape == (graph.num_nodes, 1433) and float(t.abs().sum()) > 0
    back = t.to(torch.bfloat16).float()
    assert torch.equal(back.view(torch.int32), t.view(torch.int32)), "a stand-in feature is not exact in bf16"
