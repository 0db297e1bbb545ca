"""sage_csr_sum on the GPU: the grouped row sum behind a shared embedding's gradient, against an fp64 sum at every group size at
which the kernel takes another path (empty, one wave's load, the 8-row unroll's edges, one chunk, chunk + 1, several chunks)."""
import ctypes

import numpy as np
import pytest
import torch

from sage355 import autograd, native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [0, 1, 2, 63, 64, 65, 0, 511, 512, 513, 1024, 1025, 1537, 2600, 0]
N, K = sum(SIZES), len(SIZES)
WIDTHS = [1, 4, 50, 128, 132]                                      # 1, 50: one float per lane; 4, 128, 132: 16 B per lane
U = 2.0 ** -24


@pytest.fixture(scope="module")
def csr():
    """rowptr of SIZES; col a random permutation of the N source rows; col_dup the same with repeated ids inside every group of
    two or more."""
    rng = np.random.default_rng(7)
    rowptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    col = rng.permutation(N).astype(np.int32)
    col_dup = col.copy()
    for b, e in zip(rowptr[:-1], rowptr[1:]):
        if e - b >= 2:
            col_dup[b + 1:e:3] = col_dup[b:e - 1:3][: len(col_dup[b + 1:e:3])]
    assert any(len(set(col_dup[b:e])) < e - b for b, e in zip(rowptr[:-1], rowptr[1:]))
    return rowptr, col, col_dup, torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(col_dup).to(DEV)


_tables = {}


def table_of(dim):
    if dim not in _tables:
        _tables[dim] = torch.randn(N, dim, generator=torch.Generator().manual_seed(100 + dim))
    return _tables[dim]


def reference(rowptr, col, table):
    """fp64 sums and the sums of the terms' magnitudes, per group."""
    t = table.double().numpy()
    ref, mag = np.zeros((K, t.shape[1])), np.zeros((K, t.shape[1]))
    for r in range(K):
        rows = t[col[rowptr[r]:rowptr[r + 1]]]
        ref[r], mag[r] = rows.sum(0), np.abs(rows).sum(0)
    return ref, mag


def gamma_bound(mag):
    """gamma_n * sum|terms| with n = min(m, 512) + ceil(m / 512): the worst case of any order whose longest chain of additions is
    one chunk plus the chunk adds (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    m = np.asarray(SIZES, dtype=np.float64)
    n = np.minimum(m, 512) + np.ceil(m / 512)
    return (n * U / (1 - n * U))[:, None] * mag


def check(out, ref, mag, what):
    err = np.abs(out.double().cpu().numpy() - ref)
    bound = gamma_bound(mag)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |out - ref| = {err.max():.3e}, max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{what}: |out - ref| exceeds gamma_n * sum|terms| (ratio {worst:.3f})"
    for r, m in enumerate(SIZES):
        if m == 0:
            assert not out[r].cpu().numpy().any(), f"{what}: empty group {r} is not exact zeros"


@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("dim", WIDTHS)
def test_csr_sum_matches_fp64_within_the_summation_bound(csr, dim, dup):
    rowptr, col, col_dup, rp_d, col_d, dup_d = csr
    table = table_of(dim)
    ref, mag = reference(rowptr, col_dup if dup else col, table)
    out = ops.csr_sum(rp_d, dup_d if dup else col_d, table.to(DEV))
    assert out.shape == (K, dim) and out.dtype == torch.float32
    check(out, ref, mag, f"dim {dim} dup {dup}")


@pytest.mark.parametrize("dim,pad", [(50, 3), (128, 4), (132, 8)])
def test_csr_sum_writes_every_row_and_nothing_else(csr, dim, pad):
    """ld and ldo larger than dim; out pre-filled with NaN with a canary row behind it; the workspace with a canary tail."""
    rowptr, col, _, rp_d, col_d, _ = csr
    table = table_of(dim)
    ref, mag = reference(rowptr, col, table)
    wide = torch.full((N, dim + pad), float("nan"), device=DEV)
    wide[:, :dim] = table.to(DEV)
    buf = torch.full((K + 1, dim + pad), float("nan"), device=DEV)
    need = ops.csr_sum_workspace_bytes(K, N, dim)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    out = ops.csr_sum(rp_d, col_d, wide[:, :dim], out=buf[:K, :dim], workspace=ws[:need])
    assert out.data_ptr() == buf.data_ptr()
    assert not bool(torch.isnan(buf[:K, :dim]).any()), "a row of out was not stored"
    assert bool(torch.isnan(buf[:K, dim:]).all()) and bool(torch.isnan(buf[K]).all()), "csr_sum wrote outside out[:K, :dim]"
    assert bool((ws[need:] == 0xA5).all()), "csr_sum wrote past its workspace"
    check(buf[:K, :dim], ref, mag, f"dim {dim} ld {dim + pad}")
    # the padded layout takes the same arithmetic wherever the 16-byte path is allowed in both
    if (dim + pad) % 4 == 0 and dim % 4 == 0:
        assert torch.equal(buf[:K, :dim].contiguous().view(torch.int32), ops.csr_sum(rp_d, col_d, table.to(DEV)).view(torch.int32))


@pytest.mark.parametrize("dim", [50, 128])
def test_csr_sum_bits_do_not_depend_on_the_run_or_the_workspace(csr, dim):
    rowptr, col, _, rp_d, col_d, _ = csr
    t = table_of(dim).to(DEV)
    full = ops.csr_sum(rp_d, col_d, t)
    again = ops.csr_sum(rp_d, col_d, t)
    assert torch.equal(full.view(torch.int32), again.view(torch.int32)), "two calls differ"
    # max_edges = 512: no long row's chunks fit, every one is summed by its row wave; 2048: the first three long rows fit
    for bound in (512, 2048):
        need = ops.csr_sum_workspace_bytes(K, bound, dim)
        assert need < ops.csr_sum_workspace_bytes(K, N, dim)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        small = ops.csr_sum(rp_d, col_d, t, max_edges=bound, workspace=ws[:need])
        assert torch.equal(full.view(torch.int32), small.view(torch.int32)), f"max_edges = {bound} changes the bits"
        assert bool((ws[need:] == 0xA5).all()), "csr_sum wrote past a small workspace"


def test_csr_sum_clamps_ids_into_the_table(csr):
    rowptr, col, _, rp_d, _, _ = csr
    bad = col.copy()
    bad[5], bad[700], bad[3000] = -9, N + 100, np.iinfo(np.int32).max
    t = table_of(4).to(DEV)
    got = ops.csr_sum(rp_d, torch.from_numpy(bad).to(DEV), t)
    want = ops.csr_sum(rp_d, torch.from_numpy(np.clip(bad, 0, N - 1)).to(DEV), t)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_a_refused_call_leaves_out_untouched(csr):
    _, _, _, rp_d, col_d, _ = csr
    L, P = native.lib(), native.ptr
    t = table_of(4).to(DEV)
    out = torch.full((K, 4), float("nan"), device=DEV)
    need = ops.csr_sum_workspace_bytes(K, N, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = native.stream_handle()
    assert L.sage_csr_sum(P(rp_d), P(col_d), K, N, P(t), N, 4, 4, P(out), 4, P(ws), need - 256, stream) == native.ENOSPACE
    assert L.sage_csr_sum(P(rp_d), P(col_d), K, N, P(t), N, 3, 4, P(out), 4, P(ws), need, stream) == native.EINVAL
    assert L.sage_csr_sum(P(rp_d), P(col_d), K, N, P(t), N, 4, 4, P(out), 4, ctypes.c_void_p(ws.data_ptr() + 4), need, stream) == native.EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(native.SageError):
        ops.csr_sum(rp_d, col_d, t, out=torch.empty(K, 5, device=DEV))


@pytest.mark.parametrize("dim", [50, 128])
def test_embed_rows_backward_is_csr_sum_over_the_groups(csr, dim):
    """autograd.embed_rows: the forward is index_select, the gradient of row k is the sum of the cotangent rows that read it."""
    rowptr, col, _, rp_d, col_d, _ = csr
    index = np.empty(N, dtype=np.int32)
    index[col] = np.repeat(np.arange(K), SIZES)                     # the index whose grouping is (rowptr, sorted col)
    idx_d = torch.from_numpy(index).to(DEV)
    w = torch.randn(K, dim, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    cot = table_of(dim)
    x = autograd.embed_rows(w, idx_d)
    assert torch.equal(x, w.detach()[idx_d.long()])
    (g,) = torch.autograd.grad(x, (w,), cot.to(DEV))
    rp_g, col_g = ops.group_rows(idx_d, K)
    assert torch.equal(rp_g.cpu(), torch.from_numpy(rowptr))
    ref, mag = reference(rowptr, col_g.cpu().numpy(), cot)
    check(g, ref, mag, f"embed_rows grad dim {dim}")
    x2 = autograd.embed_rows(w, idx_d, groups=(rp_g, col_g))
    (g2,) = torch.autograd.grad(x2, (w,), cot.to(DEV))
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32))
    with torch.no_grad():
        assert not autograd.embed_rows(w, idx_d).requires_grad
