"""CPU checks of the pagerank initializer (sage_pagerank_*): the symbols, argument validation before any launch, the workspace
query, the golden fixture against an fp64 restatement of nx.pagerank's iteration written here (the oracle tests/test_gpu_pagerank.py
imports), and the run drivers' act1 argument."""
import ctypes
import os
import re

import numpy as np
import pytest

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "pagerank_cases.npz")
ALPHA, TOL, MAX_ITER = 0.85, 1e-6, 100                               # nx.pagerank's defaults


def step_fp64(rowptr, col, x, inv_out, alpha=ALPHA):
    """One power-iteration step in fp64 as a PULL: row i of (rowptr, col) lists the nodes that link to i.  -> (x_next, err, mass)."""
    n = len(rowptr) - 1
    x, inv_out = np.asarray(x, dtype=np.float64), np.asarray(inv_out, dtype=np.float64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    e = int(rowptr[-1])
    s = np.bincount(rows, weights=(x * inv_out)[col[:e]], minlength=n)
    mass = x[inv_out == 0].sum()
    x_next = alpha * (s + mass / n) + (1.0 - alpha) / n
    return x_next, np.abs(x_next - x).sum(), mass


def pagerank_fp64(rowptr, col, symmetric=True, alpha=ALPHA, tol=TOL, max_iter=MAX_ITER):
    """nx.pagerank with its defaults, restated: uniform start, personalization and dangling weights, stop after the first step with
    err < N * tol.  Rows are the graph's own for a symmetric graph, out-edge lists otherwise.  -> (x, iterations, [err per step])."""
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    if not symmetric:                                                # pull over the transpose, out-degrees of the original rows
        src = np.repeat(np.arange(n), deg)
        order = np.argsort(col, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])
        col = src[order]
    inv_out = np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)
    x = np.full(n, 1.0 / n)
    errs = []
    for it in range(1, max_iter + 1):
        x, err, _ = step_fp64(rowptr, col, x, inv_out, alpha)
        errs.append(err)
        if err < n * tol:
            return x, it, errs
    raise RuntimeError("no convergence")


def golden_cases():
    z = np.load(GOLDEN)
    return {str(c): {k: z[f"{c}_{k}"] for k in ("rowptr", "col", "symmetric", "x", "iterations", "err")} for c in z["cases"]}


def test_pagerank_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in ("sage_pagerank_workspace_bytes", "sage_pagerank_init", "sage_pagerank_step", "sage_pagerank_load"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
    assert L.sage_pagerank_workspace_bytes.restype is ctypes.c_size_t
    assert native.ABI_VERSION == 9 and L.sage_abi_version() == 9     # additive


def _host_arrays():
    arr = (ctypes.c_int64 * 64)()
    return [ctypes.cast(ctypes.addressof(arr) + 32 * i, ctypes.c_void_p) for i in range(8)], arr


def test_pagerank_rejects_bad_arguments_before_any_launch():
    L = native.lib()

    def step(n=10, e=100, alpha=0.85):                               # every array NULL: whatever else is wrong, nothing can be launched
        return L.sage_pagerank_step(None, None, n, e, None, alpha, None, None, None, None, None, None, 0, None)

    def init(n=10, e=100):
        return L.sage_pagerank_init(None, n, e, None, None, None, None, None, None, 0, None)

    def load(n=10, e=100):
        return L.sage_pagerank_load(None, n, e, None, None, None, None, None, 0, None)

    for call in (step, init, load):
        assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
        for kw, word in [(dict(n=0), b"num_nodes"), (dict(n=-5), b"num_nodes"), (dict(n=1 << 31), b"num_nodes"), (dict(e=-1), b"num_edges"),
                         (dict(e=1 << 50), b"out of range")]:
            assert call(**kw) == native.EINVAL, kw
            assert word in L.sage_last_error(), (kw, L.sage_last_error())
    for alpha in (0.0, 1.0, -0.2, 1.5, float("nan")):
        assert step(alpha=alpha) == native.EINVAL and b"alpha" in L.sage_last_error(), alpha
    # arrays that are not NULL (host memory: nothing may be launched on them): aliased outputs are refused
    (rp, col, inv, x, y, xn, yn, st), keep = _host_arrays()
    assert L.sage_pagerank_step(rp, col, 4, 4, inv, 0.85, x, y, x, yn, st, None, 0, None) == native.EINVAL
    assert b"ping-pong" in L.sage_last_error()
    assert L.sage_pagerank_step(rp, col, 4, 4, inv, 0.85, x, y, xn, y, st, None, 0, None) == native.EINVAL
    assert L.sage_pagerank_init(rp, 4, 4, None, x, x, inv, st, None, 0, None) == native.EINVAL and b"three arrays" in L.sage_last_error()
    del keep


def test_pagerank_workspace_is_checked_before_any_launch():
    L = native.lib()
    (rp, col, inv, x, y, xn, yn, st), keep = _host_arrays()
    need = L.sage_pagerank_workspace_bytes(4, 4)
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256

    calls = [lambda ws, nb: L.sage_pagerank_step(rp, col, 4, 4, inv, 0.85, x, y, xn, yn, st, ctypes.c_void_p(ws), nb, None),
             lambda ws, nb: L.sage_pagerank_init(rp, 4, 4, None, x, y, inv, st, ctypes.c_void_p(ws), nb, None),
             lambda ws, nb: L.sage_pagerank_load(rp, 4, 4, x, inv, y, st, ctypes.c_void_p(ws), nb, None)]
    for call in calls:
        assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
        assert call(base, 0) == native.ENOSPACE
        assert call(None, need) == native.ENOSPACE
        assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
    del keep


def test_pagerank_workspace_query_is_host_arithmetic():
    ws = native.lib().sage_pagerank_workspace_bytes
    assert ws(0, 10) == 0 and ws(-1, 10) == 0 and ws(10, -1) == 0 and ws(1 << 31, 10) == 0 and ws(10, 1 << 50) == 0
    for n in (1, 63, 1024, 1025, 2049, 1 << 20, (1 << 31) - 1):
        for e in (0, 511, 512, 513, 10_000, 128_000_000):
            b = ws(n, e)
            assert b > 0 and b % 256 == 0, (n, e, b)
            assert ws(n + 1 if n + 1 < (1 << 31) else n, e) >= b and ws(n, e + 1) >= b, (n, e)
    assert ws(1, 100 * 512) - ws(1, 0) >= 100 * 4                    # one float per chunk of a long row
    assert ws(1 << 20, 0) >= (1 << 20) * 8 + 2 * 2048 * 4             # the plan's offsets and one (err, mass) pair per 512 rows
    assert ops.pagerank_workspace_bytes(1 << 20, 1 << 24) == ws(1 << 20, 1 << 24)


def test_fp64_restatement_reproduces_the_golden_fixture():
    cases = golden_cases()
    assert sorted(cases) == ["a", "b", "c", "d"]
    for name, c in cases.items():
        n = len(c["rowptr"]) - 1
        x, it, errs = pagerank_fp64(c["rowptr"], c["col"], symmetric=bool(c["symmetric"]))
        assert it == int(c["iterations"]), name
        assert float((np.abs(x - c["x"]) / c["x"]).max()) <= 1e-12, name
        assert np.allclose(errs[-2:], c["err"], rtol=1e-9, atol=0), name
        assert errs[-1] <= 0.99 * n * TOL and errs[-2] >= 1.01 * n * TOL, name     # an fp32 err cannot land on the other side
        assert abs(x.sum() - 1.0) <= 1e-12
    lens = np.diff(cases["b"]["rowptr"])
    assert lens.max() > 2 * native.CSR_MEAN_CHUNK and (lens == 0).sum() >= 40 and bool(cases["a"]["symmetric"]) and not bool(cases["d"]["symmetric"])
    d = cases["d"]
    assert (np.diff(d["rowptr"]) == 0).any(), "case d needs a sink"


def test_ops_refuse_bad_pagerank_arguments_on_the_host():
    import torch
    rp, col = torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(native.SageError):
        ops.pagerank(rp, col)                                        # no GPU / host tensors: never a launch on host memory
    with pytest.raises(native.SageError):
        ops.pagerank_step(rp, col, torch.ones(2), torch.ones(2))


@pytest.mark.parametrize("driver", ["engine", "exact_batch", "full_graph"])
def test_run_drivers_refuse_act1_with_an_initializer_that_sets_its_own(driver):
    from sage355 import exactbatch, fullgraph, train
    from sage355.graph import csr_from_edges
    run = {"engine": train.run_engine_training, "exact_batch": exactbatch.run_exact_batch_training,
           "full_graph": fullgraph.run_full_graph_training}[driver]
    g = csr_from_edges([0, 1, 2], [1, 2, 3], 4)
    labels = np.zeros((4, 1), dtype=np.int64)
    for initializer in ("node_degree", "1hot"):
        with pytest.raises(native.SageError, match="act1"):
            run(g, None, labels, 2, initializer=initializer, act1=native.ACT_SIGMOID)
    with pytest.raises(native.SageError, match="initializer"):      # the refusal that was there stays what it was
        run(g, None, labels, 2, initializer="pagerank", act1=native.ACT_SIGMOID)
