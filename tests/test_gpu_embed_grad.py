"""sage_embed_grad on the GPU, the kernel alone: the gradient of an embedding through sampled sets that hold embedding rows, against
an fp64 sum at every run length at which the kernel takes another path (empty, one trip of 8, one chunk, chunk + 1, several chunks);
its independence of where the rows lie; the live-row count; what it writes and what it leaves alone."""
import ctypes

import numpy as np
import pytest
import torch

from sage355 import native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [0, 1, 2, 63, 64, 65, 0, 511, 512, 513, 1024, 1025, 1537, 2600, 0]        # terms per embedding row: tests/test_gpu_csr_sum.py's
R, TERMS = len(SIZES), sum(SIZES)
FANOUTS = [1, 7, 64]
WIDTHS = [4, 52, 128, 132]
U = 2.0 ** -24

_cases = {}


def case(k):
    """(nodes, nbr [n, k], cnt [n]) on the host: the multiset of keys (embedding row e SIZES[e] times), permuted and cut into rows of
    k slots.  Row fills cycle through k, k, 0, 1, k - 1 and k with cnt = k + 3 (cnt > k: the kernel takes k); padding is -1."""
    if k not in _cases:
        rng = np.random.default_rng(40 + k)
        keys = rng.permutation(np.repeat(np.arange(R), SIZES)).astype(np.int32)
        fills = [(k, k), (k, k), (0, 0), (min(1, k), min(1, k)), (k - 1, k - 1), (k, k + 3)]      # (terms held, cnt stored)
        rows, cnts, pos, i = [], [], 0, 0
        while pos < TERMS:
            held, stored = fills[i % len(fills)]
            i += 1
            held = min(held, TERMS - pos)
            if held < min(stored, k):
                stored = held
            row = np.full(k, -1, dtype=np.int32)
            row[:held] = keys[pos:pos + held]
            pos += held
            rows.append(row)
            cnts.append(stored)
        nbr, cnt = np.stack(rows), np.asarray(cnts, dtype=np.int32)
        n = len(cnt)
        assert {0, min(1, k), k - 1, k + 3} <= set(cnt.tolist()) and n >= 2 * 64
        nodes = rng.permutation(10 * n)[:n].astype(np.int32)                                     # distinct node ids, in no order
        held = np.minimum(cnt, k)
        assert np.array_equal(np.bincount(np.concatenate([nbr[t, :held[t]] for t in range(n)]), minlength=R), SIZES)
        _cases[k] = (nodes, nbr, cnt)
    return _cases[k]


_grads, _refs = {}, {}


def grad_of(k, dim):
    if (k, dim) not in _grads:
        n = case(k)[1].shape[0]
        _grads[(k, dim)] = torch.randn(n, dim, generator=torch.Generator().manual_seed(1000 * k + dim))
    return _grads[(k, dim)]


def reference(k, dim):
    """fp64 sums of grad_agg[t] / c_t per embedding row, and the sums of the terms' magnitudes."""
    if (k, dim) not in _refs:
        _, nbr, cnt = case(k)
        g = grad_of(k, dim).double().numpy()
        ref, mag = np.zeros((R, dim)), np.zeros((R, dim))
        for t in range(nbr.shape[0]):
            c = min(int(cnt[t]), k)
            for j in range(c):
                e = int(nbr[t, j])
                ref[e] += g[t] / c
                mag[e] += np.abs(g[t]) / c
        _refs[(k, dim)] = (ref, mag)
    return _refs[(k, dim)]


def check(out, ref, mag, what):
    """gamma_m * sum|terms|, m = min(c, 512) + ceil(c / 512) + 1 for a row of c terms: the longest chain of additions is one chunk
    plus the chunk adds (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; tests/test_gpu_csr_sum.py's bound) and
    one rounding more for the weight 1 / c_t."""
    c = np.asarray(SIZES, dtype=np.float64)
    m = np.minimum(c, 512) + np.ceil(c / 512) + 1
    bound = (m * U / (1 - m * U))[:, None] * mag
    err = np.abs(out.double().cpu().numpy() - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |out - ref| = {err.max():.3e}, max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{what}: |out - ref| exceeds gamma_m * sum|terms| (ratio {worst:.3f})"
    for e, size in enumerate(SIZES):
        if size == 0:
            assert not out[e].cpu().numpy().any(), f"{what}: embedding row {e} without a term is not exact zeros"


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("k", FANOUTS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_embed_grad_matches_fp64_within_the_summation_bound(dim, k):
    _, nbr, cnt = case(k)
    nbr_d, cnt_d = dev(nbr, cnt)
    out = ops.embed_grad(grad_of(k, dim).to(DEV), nbr_d, cnt_d, R)
    assert out.shape == (R, dim) and out.dtype == torch.float32
    check(out, *reference(k, dim), f"dim {dim} k {k}")
    again = ops.embed_grad(grad_of(k, dim).to(DEV), nbr_d, cnt_d, R)
    assert torch.equal(bits(out), bits(again)), "two calls differ"


@pytest.mark.parametrize("k", FANOUTS)
@pytest.mark.parametrize("dim", [52, 128])
def test_embed_grad_bits_do_not_depend_on_where_the_rows_lie(dim, k):
    """The n rows of (nodes, nbr, cnt, grad_agg) permuted together, each layout summed in ops.row_order's order of its node ids."""
    nodes, nbr, cnt = case(k)
    g = grad_of(k, dim)
    n = len(cnt)
    nodes_d, nbr_d, cnt_d = dev(nodes, nbr, cnt)
    order_a = ops.row_order(nodes_d)
    assert np.array_equal(order_a.cpu().numpy(), np.argsort(nodes, kind="stable"))
    a = ops.embed_grad(g.to(DEV), nbr_d, cnt_d, R, row_order=order_a)
    check(a, *reference(k, dim), f"row_order dim {dim} k {k}")
    perm = np.random.default_rng(5).permutation(n)
    nodes_p, nbr_p, cnt_p = dev(nodes[perm], nbr[perm], cnt[perm])
    b = ops.embed_grad(g[torch.from_numpy(perm)].to(DEV), nbr_p, cnt_p, R, row_order=ops.row_order(nodes_p))
    assert torch.equal(bits(a), bits(b)), f"{int((bits(a) != bits(b)).sum())} elements differ between two layouts of the same rows"


@pytest.mark.parametrize("k,dim", [(7, 52), (64, 128)])
def test_rows_past_the_live_count_add_nothing(k, dim):
    """n_dev below n against the call on the truncated arrays, bit for bit, with and without a row order."""
    nodes, nbr, cnt = case(k)
    g = grad_of(k, dim).to(DEV)
    n = len(cnt)
    live = n - n // 3
    nodes_d, nbr_d, cnt_d = dev(nodes, nbr, cnt)
    n_dev = torch.tensor([live], dtype=torch.int32, device=DEV)
    want = ops.embed_grad(g[:live].contiguous(), nbr_d[:live].contiguous(), cnt_d[:live].contiguous(), R)
    got = ops.embed_grad(g, nbr_d, cnt_d, R, n_dev=n_dev)
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(bits(got), bits(ops.embed_grad(g, nbr_d, cnt_d, R))), "the dead rows hold terms: the full call must differ"
    want_o = ops.embed_grad(g[:live].contiguous(), nbr_d[:live].contiguous(), cnt_d[:live].contiguous(), R,
                            row_order=ops.row_order(nodes_d[:live].contiguous()))
    got_o = ops.embed_grad(g, nbr_d, cnt_d, R, n_dev=n_dev, row_order=ops.row_order(nodes_d, n_dev=n_dev))
    assert torch.equal(bits(got_o), bits(want_o))
    beyond = torch.tensor([n + 1000], dtype=torch.int32, device=DEV)                              # min(*n_dev, n)
    assert torch.equal(bits(ops.embed_grad(g, nbr_d, cnt_d, R, n_dev=beyond)), bits(ops.embed_grad(g, nbr_d, cnt_d, R)))


@pytest.mark.parametrize("k,dim,pad", [(7, 52, 4), (64, 128, 8), (1, 132, 4)])
def test_embed_grad_writes_every_row_and_nothing_else(k, dim, pad):
    """ldg and ld larger than dim with NaN in the pad columns; a NaN row behind grad_embed; a canary tail behind the workspace; a
    workspace 256 bytes short is refused and nothing is written."""
    _, nbr, cnt = case(k)
    nbr_d, cnt_d = dev(nbr, cnt)
    n = len(cnt)
    wide = torch.full((n, dim + pad), float("nan"), device=DEV)
    wide[:, :dim] = grad_of(k, dim).to(DEV)
    buf = torch.full((R + 1, dim + pad), float("nan"), device=DEV)
    need = ops.embed_grad_workspace_bytes(n, k, R, dim)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    L, P = native.lib(), native.ptr
    rc = L.sage_embed_grad(P(wide), dim + pad, dim, P(nbr_d), P(cnt_d), k, n, None, None, P(buf), R, dim + pad, P(ws), need - 256,
                           native.stream_handle())
    assert rc == native.ENOSPACE
    rc = L.sage_embed_grad(P(wide), dim + pad, dim, P(nbr_d), P(cnt_d), k, n, None, None, P(buf), R, dim + pad,
                           ctypes.c_void_p(ws.data_ptr() + 4), need, native.stream_handle())
    assert rc == native.EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool((ws == 0xA5).all()), "a refused call wrote something"
    out = ops.embed_grad(wide[:, :dim], nbr_d, cnt_d, R, out=buf[:R, :dim], workspace=ws[:need])
    assert out.data_ptr() == buf.data_ptr()
    assert not bool(torch.isnan(buf[:R, :dim]).any()), "a row of grad_embed was not stored"
    assert bool(torch.isnan(buf[:R, dim:]).all()) and bool(torch.isnan(buf[R]).all()), "embed_grad wrote outside grad_embed[:R, :dim]"
    assert bool((ws[need:] == 0xA5).all()), "embed_grad wrote past its workspace"
    check(buf[:R, :dim], *reference(k, dim), f"dim {dim} ld {dim + pad} k {k}")
    assert torch.equal(bits(buf[:R, :dim]), bits(ops.embed_grad(grad_of(k, dim).to(DEV), nbr_d, cnt_d, R))), "the padded layout changes the bits"


def test_embed_grad_clamps_ids_into_the_embedding():
    """One id below 0 and one at embed_rows land on rows 0 and embed_rows - 1 (both without a term otherwise)."""
    k, dim = 7, 52
    _, nbr, cnt = case(k)
    g = grad_of(k, dim).to(DEV)
    bad = nbr.copy()
    assert cnt[0] == k and cnt[1] == k and SIZES[0] == 0 and SIZES[-1] == 0
    bad[0, 2], bad[1, 5] = -9, R
    nbr_d, bad_d, clip_d, cnt_d = dev(nbr, bad, np.clip(bad, 0, R - 1), cnt)
    got = ops.embed_grad(g, bad_d, cnt_d, R)
    assert torch.equal(bits(got), bits(ops.embed_grad(g, clip_d, cnt_d, R)))
    assert torch.equal(got[0], g[0] * (1.0 / k)) and torch.equal(got[R - 1], g[1] * (1.0 / k))   # one term each: fma(g, 1 / c, 0)
    base = ops.embed_grad(g, nbr_d, cnt_d, R)
    assert not base[0].any() and not base[R - 1].any()


def test_the_wrapper_refuses_shapes_that_do_not_fit():
    _, nbr, cnt = case(7)
    nbr_d, cnt_d = dev(nbr, cnt)
    g = grad_of(7, 52).to(DEV)
    with pytest.raises(native.SageError):
        ops.embed_grad(g, nbr_d, cnt_d, R, out=torch.empty(R, 56, device=DEV))
    with pytest.raises(native.SageError):
        ops.embed_grad(g[:10], nbr_d, cnt_d, R)
    with pytest.raises(native.SageError):
        ops.embed_grad(g, nbr_d, cnt_d, R, row_order=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(native.SageError):
        ops.embed_grad(g, nbr_d.long(), cnt_d, R)
    assert not ops.embed_grad(g[:0], nbr_d[:0], cnt_d[:0], R).any()                               # no sets: zeros, written by the wrapper
