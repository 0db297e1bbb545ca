"""CPU checks of the eigen_decomposition initializer (sage_csr_cheb_*, ops.eigen_top): the symbols, argument validation before any
launch, the workspace query, the golden fixture against an fp64 eigh restated here (the loader tests/test_gpu_eigen.py imports), the
refusals of the ops wrappers without a GPU, and the run drivers' initializer argument."""
import ctypes
import os
import re

import numpy as np
import pytest

from sage355 import native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(REPO, "tests", "golden")
TOL = 3e-5                                                           # the tolerance the GPU tests run at (make_golden_eigen.py)
ENTRIES = ("sage_csr_cheb_workspace_bytes", "sage_csr_cheb_plan", "sage_csr_cheb_step")


def golden_cases():
    """{case: dict(rowptr, col, k, values [k + 1], vectors [N, k])} of tests/golden/eigen_cases.npz; the Cora case's CSR comes from
    cora_topology.npz and its vectors from the column parts eigen_cases_cora_<i>.npz."""
    z = np.load(os.path.join(GOLDEN_DIR, "eigen_cases.npz"))
    out = {}
    for c in (str(c) for c in z["cases"]):
        k = int(z[f"{c}_k"])
        if str(z[f"{c}_graph"]) == "cora":
            topo = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
            rowptr, col = topo["rowptr"].astype(np.int64), topo["col"].astype(np.int32)
            vectors = np.zeros((len(rowptr) - 1, k))
            filled = 0
            for i in range(3):
                part = np.load(os.path.join(GOLDEN_DIR, f"eigen_cases_cora_{i}.npz"))
                first, v = int(part["first"]), part["vectors"]
                assert first == filled
                vectors[:, first:first + v.shape[1]] = v
                filled += v.shape[1]
            assert filled == k
        else:
            rowptr, col, vectors = z[f"{c}_rowptr"], z[f"{c}_col"], z[f"{c}_vectors"]
        out[c] = dict(rowptr=rowptr, col=col, k=k, values=z[f"{c}_values"], vectors=vectors)
    return out


def dense_adjacency(rowptr, col):
    """float64 [N, N]: every stored entry a 1 (the fixtures hold no duplicate entry)."""
    n = len(rowptr) - 1
    a = np.zeros((n, n))
    a[np.repeat(np.arange(n), np.diff(rowptr)), col[:int(rowptr[-1])]] = 1.0
    return a


def test_csr_cheb_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sage355.h")).read(), flags=re.S)
    L = native.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/sage355.h"
        assert name in native.SYMBOLS and hasattr(L, name)
    assert L.sage_csr_cheb_workspace_bytes.restype is ctypes.c_size_t
    assert native.ABI_VERSION == 9 and L.sage_abi_version() == 9     # additive
    for name in ("csr_cheb_workspace_bytes", "csr_cheb_plan", "csr_cheb_step", "CsrChebPlan", "eigen_top"):
        assert hasattr(ops, name), name
    from sage355 import datasets
    assert callable(datasets.eigen_table)


def _host_arrays():
    arr = (ctypes.c_int64 * 4096)()                                   # 32 KiB: four 8 KiB arrays, 16-byte aligned steps
    base = (ctypes.addressof(arr) + 15) // 16 * 16
    return [base + 8000 * i for i in range(4)], arr


def _step(L, rowptr, col, y, x, out, n=4, e=4, ldy=8, ldx=8, dim=8, ldo=8, ws=None, nb=0):
    vp = lambda a: None if a is None else ctypes.c_void_p(a)         # noqa: E731
    return L.sage_csr_cheb_step(vp(rowptr), vp(col), n, e, vp(y), ldy, vp(x), ldx, dim, 1.0, 0.5, -0.25, vp(out), ldo, vp(ws), nb, None)


def test_csr_cheb_rejects_bad_arguments_before_any_launch():
    L = native.lib()

    def step(**kw):                                                   # every array NULL: whatever else is wrong, nothing can be launched
        return _step(L, None, None, None, None, None, **kw)

    def plan(n=4, e=4, dim=8):
        return L.sage_csr_cheb_plan(None, n, e, dim, None, 0, None)

    for call in (step, plan):
        assert call() == native.EINVAL and b"NULL" in L.sage_last_error()
        for kw, word in [(dict(n=0), b"num_nodes"), (dict(n=-5), b"num_nodes"), (dict(n=1 << 31), b"num_nodes"), (dict(e=-1), b"num_edges"),
                         (dict(dim=0), b"dim"), (dict(dim=-4), b"dim"), (dict(dim=(1 << 20) + 1), b"dim"), (dict(e=1 << 50), b"out of range")]:
            assert call(**kw) == native.EINVAL, kw
            assert word in L.sage_last_error(), (kw, L.sage_last_error())
    for kw in (dict(ldy=7), dict(ldo=7), dict(ldy=0), dict(ldo=-8)):
        assert step(**kw) == native.EINVAL and b"ld" in L.sage_last_error(), kw
    # arrays that are not NULL (host memory: nothing may be launched on them)
    (rp, col, y, x), keep = _host_arrays()
    assert _step(L, rp, col, y, x, x, ldx=7) == native.EINVAL and b"ldx" in L.sage_last_error()      # ldx counts only with an x
    assert _step(L, rp, col, y, None, x, ldx=0) == native.ENOSPACE                                   # ... and not without one
    for miss in range(3):                                             # rowptr, col, y NULL in turn; then out
        args = [rp, col, y]
        args[miss] = None
        assert _step(L, *args, None, x) == native.EINVAL and b"NULL" in L.sage_last_error()
    assert _step(L, rp, col, y, None, None) == native.EINVAL and b"NULL" in L.sage_last_error()
    # out overlapping y: the same array, a shifted view, the last element of y
    assert _step(L, rp, col, y, None, y) == native.EINVAL and b"overlaps y" in L.sage_last_error()
    assert _step(L, rp, col, y, x, y + 16) == native.EINVAL and b"overlaps y" in L.sage_last_error()
    assert _step(L, rp, col, y, x, y + (3 * 8 + 7) * 4) == native.EINVAL and b"overlaps y" in L.sage_last_error()
    assert _step(L, rp, col, y, x, y - (3 * 8 + 7) * 4) == native.EINVAL and b"overlaps y" in L.sage_last_error()
    assert _step(L, rp, col, y, x, x + 16) == native.EINVAL and b"overlaps x" in L.sage_last_error()
    # out == x is the in-place form: accepted up to the workspace check; so is an out that ends where y begins
    assert _step(L, rp, col, y, x, x) == native.ENOSPACE and b"workspace" in L.sage_last_error()
    assert _step(L, rp, col, y, None, y - (3 * 8 + 8) * 4) == native.ENOSPACE
    assert _step(L, rp, col, y, None, y + (3 * 8 + 8) * 4) == native.ENOSPACE
    del keep


def test_csr_cheb_workspace_is_checked_before_any_launch():
    L = native.lib()
    (rp, col, y, x), keep = _host_arrays()
    need = L.sage_csr_cheb_workspace_bytes(4, 4, 8)
    buf = (ctypes.c_char * (need + 512))()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    calls = [lambda ws, nb: _step(L, rp, col, y, x, x, ws=ws, nb=nb),
             lambda ws, nb: _step(L, rp, col, y, None, x, ws=ws, nb=nb),
             lambda ws, nb: L.sage_csr_cheb_plan(ctypes.c_void_p(rp), 4, 4, 8, None if ws is None else ctypes.c_void_p(ws), nb, None)]
    for call in calls:
        assert call(base, need - 256) == native.ENOSPACE and b"workspace" in L.sage_last_error()
        assert call(base, 0) == native.ENOSPACE
        assert call(None, need) == native.ENOSPACE
        assert call(base + 4, need) == native.EINVAL and b"aligned" in L.sage_last_error()
    del keep


def test_csr_cheb_workspace_query_is_host_arithmetic():
    ws = native.lib().sage_csr_cheb_workspace_bytes
    assert ws(0, 10, 8) == 0 and ws(-1, 10, 8) == 0 and ws(10, -1, 8) == 0 and ws(1 << 31, 10, 8) == 0 and ws(10, 1 << 50, 8) == 0
    assert ws(10, 10, 0) == 0 and ws(10, 10, -1) == 0 and ws(10, 10, (1 << 20) + 1) == 0
    for n in (1, 63, 1024, 2049, 1 << 20, (1 << 31) - 1):
        for e in (0, 511, 512, 513, 10_000, 128_000_000):
            for dim in (1, 4, 100, 120, 1004):
                b = ws(n, e, dim)
                assert b > 0 and b % 256 == 0, (n, e, dim, b)
                assert ws(min(n + 1, (1 << 31) - 1), e, dim) >= b and ws(n, e + 1, dim) >= b and ws(n, e, dim + 1) >= b, (n, e, dim)
    assert ws(1, 100 * 512, 120) - ws(1, 0, 120) >= 100 * 120 * 4        # a row of dim floats per chunk of a long row
    assert ws(1 << 20, 0, 4) >= (1 << 20) * 8                            # the plan's offsets
    assert ops.csr_cheb_workspace_bytes(1 << 20, 1 << 24, 120) == ws(1 << 20, 1 << 24, 120)


@pytest.fixture(scope="module")
def cases():
    return golden_cases()


def test_golden_fixture_against_an_fp64_eigh(cases):
    """The fixture is LA.eig's output (the reference's call); here numpy's symmetric solver restates it: the values to 1e-10, the
    vectors as eigenvectors to 1e-10, and the three conditions make_golden_eigen.py asserts, which tests/test_gpu_eigen.py needs."""
    assert list(cases) == ["a", "b", "b32", "c", "cora"]
    assert [cases[c]["k"] for c in cases] == [4, 8, 32, 16, 100]
    assert np.array_equal(cases["b"]["col"], cases["b32"]["col"])
    for name, c in cases.items():
        a, k, lam, u = dense_adjacency(c["rowptr"], c["col"]), c["k"], c["values"], c["vectors"]
        n = a.shape[0]
        assert np.array_equal(a, a.T) and int(a.sum()) == len(c["col"]), name
        w = np.linalg.eigvalsh(a)[::-1]
        assert lam.shape == (k + 1,) and u.shape == (n, k) and lam.dtype == np.float64 and u.dtype == np.float64
        assert float(np.abs(w[:k + 1] - lam).max()) <= 1e-10, name
        assert np.all(np.diff(lam) <= 0)
        assert float(np.abs(a @ u - u * lam[:k]).max()) <= 1e-10, name
        assert float(np.abs(np.linalg.norm(u, axis=0) - 1).max()) <= 1e-12, name
        gap, need = lam[k - 1] - lam[k], 2 * np.sqrt(k) * TOL * lam[0]
        print(f"{name}: N={n} k={k} lambda_1={lam[0]:.6f} lambda_k={lam[k - 1]:.6f} gap={gap:.3e} needed {need:.3e} ({gap / need:.2f}x)")
        assert gap >= need and lam[k - 1] > 0, name
    lens = np.diff(cases["b"]["rowptr"])
    assert lens.max() > 2 * native.CSR_MEAN_CHUNK and (lens == 0).sum() >= 40           # a chunked row and isolated nodes
    for f in os.listdir(GOLDEN_DIR):
        if f.startswith("eigen_cases"):
            assert os.path.getsize(os.path.join(GOLDEN_DIR, f)) < (1 << 20), f


def test_ops_refuse_host_tensors_and_bad_arguments_without_a_gpu():
    import torch
    rp, col = torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(native.SageError):
        ops.csr_cheb_plan(rp, col, 4)                                 # no GPU / host tensors: never a launch on host memory
    plan = ops.CsrChebPlan(rp, col, 4, 2, 2, torch.zeros(4096, dtype=torch.uint8))
    with pytest.raises(native.SageError):
        ops.csr_cheb_step(plan, torch.ones(2, 4))
    with pytest.raises(native.SageError):
        ops.csr_cheb_step(object(), torch.ones(2, 4))
    with pytest.raises(native.SageError):
        ops.eigen_top(rp, col, 1)
    for k in (0, -3, 1001):                                           # the reference asserts feature_dim <= 1000
        with pytest.raises(native.SageError, match="k = "):
            ops.eigen_top(rp, col, k)
    with pytest.raises(native.SageError, match="max_iter"):
        ops.eigen_top(rp, col, 1, max_iter=0)
    with pytest.raises(native.SageError, match="tol"):
        ops.eigen_top(rp, col, 1, tol=0.0)
    with pytest.raises(native.SageError, match="guard"):
        ops.eigen_top(rp, col, 1, guard=-1)
    from sage355.datasets import eigen_table
    from sage355.graph import csr_from_edges
    with pytest.raises(native.SageError):
        eigen_table(csr_from_edges([0, 1, 2], [1, 2, 3], 4), "cpu", 2)


@pytest.mark.parametrize("driver", ["engine", "exact_batch", "full_graph"])
def test_run_drivers_still_refuse_the_initializer_string(driver):
    """The table is made by datasets.eigen_table and handed in as feat_data; the drivers' initializer= names trainable embeddings only."""
    from sage355 import exactbatch, fullgraph, train
    from sage355.graph import csr_from_edges
    run = {"engine": train.run_engine_training, "exact_batch": exactbatch.run_exact_batch_training,
           "full_graph": fullgraph.run_full_graph_training}[driver]
    g = csr_from_edges([0, 1, 2], [1, 2, 3], 4)
    with pytest.raises(native.SageError, match="initializer"):
        run(g, None, np.zeros((4, 1), dtype=np.int64), 2, initializer="eigen_decomposition")
