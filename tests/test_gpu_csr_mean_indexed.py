"""sage_csr_mean_indexed and sage_csr_mean_backward_grouped (include/sage355.h) on the MI355X.

Forward: ops.csr_mean(embed, index=ix) against ops.csr_mean(embed[ix]) BIT FOR BIT -- the comparison kernel is the one
tests/test_gpu_csr_mean.py holds to fp64, so no tolerance is involved.

Backward: against an fp64 reference built on the CPU from the documented formula with the forward's own float weights, at the
tolerance of tests/test_gpu_csr_mean_backward.py: |got - want| <= 1e-5 * A elementwise, A the fp64 sum of the terms' absolute
values; exact zeros where A = 0; max |err| / max |want| <= 2e-5.  (The worst case gamma_n * A with n = min(m, 512) + ceil(m / 512)
is 4.5e-5 * A at the all-zero index's 116,828 terms; the kernel's order emulated in fp32 on the CPU errs by 2-5e-8 * A.)

Graphs: "sym" (the skewed graph of tests/test_gpu_csr_mean_backward.py with its reverse, n = 12,288; generator copied in
tests/test_csr_mean_indexed_host.py) and "rev" (transposed rows of exactly 0, 1, E-1, E, E+1, 2E, 2E+1 and 20E+37 entries).
With the degree index the grouped rows are empty (10,257 of them), of one to two chunks, and above two chunks (17); with the
all-zero index there is one row of 104,554 / 116,828 terms."""
import numpy as np
import pytest
import torch

from sage355 import autograd, native, ops
from test_csr_mean_indexed_host import skewed_graph, sym_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = native.CSR_MEAN_CHUNK
BOUND, MAXREL = 1e-5, 2e-5
SENTINEL = -31.5


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Graph:
    """A forward CSR on the device and the fp64 ingredients of the backward's formula."""

    def __init__(self, rowptr, col):
        self.rowptr, self.col = rowptr, col
        self.n = len(rowptr) - 1
        self.deg = np.diff(rowptr)
        self.src = np.repeat(np.arange(self.n), self.deg)
        self.own = np.zeros(self.n, dtype=bool)                         # v is an entry of its own row
        self.own[self.src[col == self.src]] = True
        self.rp_d, self.col_d = torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV)
        self._grouped = {}

    def index(self, kind):
        """(index int64 numpy [n], K)"""
        n = self.n
        return {"identity": (np.arange(n), n), "degree": (self.deg.astype(np.int64), int(self.deg.max()) + 1),
                "zero": (np.zeros(n, dtype=np.int64), 3), "last": (np.full(n, 36, dtype=np.int64), 37)}[kind]

    def index_dev(self, kind):
        ix, k = self.index(kind)
        return torch.from_numpy(ix.astype(np.int32)).to(DEV), k

    def grouped(self, kind, self_loop):
        key = (kind, self_loop)
        if key not in self._grouped:
            ix, k = self.index_dev(kind)
            self._grouped[key] = ops.csr_transpose_grouped(self.rp_d, self.col_d, ix, k, self_loop=self_loop)   # torch ops on the GPU
        return self._grouped[key]

    def weights(self, self_loop):
        extra = (~self.own) if self_loop else np.zeros(self.n, dtype=bool)
        c = self.deg + extra
        w = np.zeros(self.n, dtype=np.float32)
        w[c > 0] = np.float32(1.0) / c[c > 0].astype(np.float32)        # the forward's own float
        return extra, torch.from_numpy(w.astype(np.float64))

    def reference(self, g, kind, self_loop):
        """(want, A) fp64 [K, dim]: every entry (v -> u) of the forward puts w_v g_v onto row index[u], every node u that joined
        its own mean w_u g_u onto row index[u]."""
        ix, k = self.index(kind)
        ix = torch.from_numpy(ix)
        extra, w = self.weights(self_loop)
        term = g.double() * w[:, None]
        src, dst = torch.from_numpy(self.src), torch.from_numpy(self.col.astype(np.int64))
        want = torch.zeros(k, g.shape[1], dtype=torch.float64).index_add_(0, ix[dst], term[src])
        A = torch.zeros(k, g.shape[1], dtype=torch.float64).index_add_(0, ix[dst], term[src].abs())
        ex = torch.from_numpy(extra)
        want.index_add_(0, ix[ex], term[ex])
        A.index_add_(0, ix[ex], term[ex].abs())
        return want, A

    def run(self, g_dev, kind, self_loop, **kw):
        return ops.csr_mean_backward_grouped(self.rp_d, self.col_d, self.grouped(kind, self_loop), g_dev, **kw)


@pytest.fixture(scope="module")
def graphs():
    rowptr, col = skewed_graph()
    rp_t, c_t = ops.csr_transpose(torch.from_numpy(rowptr), torch.from_numpy(col))
    gs = {"sym": Graph(*sym_graph()), "rev": Graph(rp_t.numpy(), c_t.numpy())}
    s = gs["sym"]
    assert s.n == 24 * E and s.deg.max() > 20 * E and (s.deg == 0).any() and s.own.any()
    return gs


def _check(got, want, A, what):
    got = got.double().cpu()
    zero = A == 0
    assert bool((got[zero] == 0).all()), f"{what}: elements with no terms are not 0"
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in the result"
    err = (got - want).abs()
    tol = BOUND * A
    bad = err > tol
    print(f"{what}: max err / A = {float((err / A.clamp_min(1e-300))[~zero].max()):.3g}, max err / max|want| = {float(err.max() / want.abs().max()):.3g}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements over the bound; worst {float((err - tol).max()):.3g}"
    assert float(err.max()) / float(want.abs().max()) <= MAXREL, f"{what}: max relative error {float(err.max()) / float(want.abs().max()):.3g}"


def _grad(n, dim, pad, seed):
    """grad_out [n, dim] on the CPU and its device copy with leading dimension dim + pad."""
    wide = torch.randn(n, dim + pad, generator=torch.Generator().manual_seed(seed))
    return wide[:, :dim].contiguous(), (wide.to(DEV)[:, :dim] if pad else wide.to(DEV))


# ------------------------------------------------------------------------------------------------------------ forward
def _variants(gr):
    n = gr.n
    rng = np.random.default_rng(3)
    nodes = np.concatenate([[7, 7, -1, n, 0, 9, 9, n - 1, 1 << 30], rng.integers(0, n, 300)]).astype(np.int32)   # the hub twice, ids outside
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    return [dict(), dict(nodes=torch.from_numpy(nodes).to(DEV)), dict(any_nonempty=one), dict(max_edges=512), dict(max_edges=2048),
            dict(nodes=torch.from_numpy(nodes).to(DEV), any_nonempty=one, max_edges=0)]


@pytest.mark.parametrize("dim", [64, 260, 50, 70])
@pytest.mark.parametrize("kind", ["identity", "degree", "zero", "last"])
def test_indexed_forward_is_the_materialised_forward_bit_for_bit(graphs, kind, dim):
    gr = graphs["sym"]
    ix, k = gr.index_dev(kind)
    embed = torch.randn(k, dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(dim))
    table = embed[ix.long()]
    for self_loop in (False, True):
        for kw in _variants(gr):
            want = ops.csr_mean(gr.rp_d, gr.col_d, table, self_loop=self_loop, **kw)
            got = ops.csr_mean(gr.rp_d, gr.col_d, embed, self_loop=self_loop, index=ix, **kw)
            assert bits_equal(got, want), (kind, dim, self_loop, sorted(kw))
            if "any_nonempty" in kw and not self_loop:
                assert bool(torch.isnan(got).any()), "the NaN rule was not exercised"


@pytest.mark.parametrize("dim", [64, 50])
def test_indexed_forward_with_a_padded_embedding_and_a_padded_out(graphs, dim):
    """ld = dim + 1 forces the scalar path; the sentinel columns and rows of a wider, longer `out` stay untouched."""
    gr = graphs["sym"]
    ix, k = gr.index_dev("degree")
    wide = torch.randn(k, dim + 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    embed = wide[:, :dim]
    assert embed.stride(0) == dim + 1
    for self_loop in (False, True):
        want = ops.csr_mean(gr.rp_d, gr.col_d, embed.contiguous()[ix.long()], self_loop=self_loop)
        assert bits_equal(ops.csr_mean(gr.rp_d, gr.col_d, embed, self_loop=self_loop, index=ix), want)
        assert bits_equal(ops.csr_mean(gr.rp_d, gr.col_d, wide[ix.long()][:, :dim], self_loop=self_loop), want)
        big = torch.full((gr.n + 5, dim + 4), SENTINEL, device=DEV)
        ops.csr_mean(gr.rp_d, gr.col_d, embed.contiguous(), self_loop=self_loop, index=ix, out=big[:, :dim])
        assert bits_equal(big[:gr.n, :dim], want)
        assert bool((big[:, dim:] == SENTINEL).all()) and bool((big[gr.n:] == SENTINEL).all()), "padding columns or rows past n written"


def test_indexed_forward_clamps_the_index_and_decides_the_self_term_on_node_ids(graphs):
    gr = graphs["sym"]
    n, dim, k = gr.n, 64, 11
    embed = torch.randn(k, dim, device=DEV)
    raw = torch.randint(-5, k + 5, (n,), dtype=torch.int32, device=DEV)
    clamped = raw.clamp(0, k - 1)
    assert bool((raw != clamped).any())
    for self_loop in (False, True):
        assert bits_equal(ops.csr_mean(gr.rp_d, gr.col_d, embed, self_loop=self_loop, index=raw),
                          ops.csr_mean(gr.rp_d, gr.col_d, embed[clamped.long()], self_loop=self_loop))
    # an all-zero index makes every index value equal every other: whether row v holds v must still come from the node ids.
    # Row 8 holds node 8 (no extra term, count = deg), row 4 does not (count = deg + 1); every term is embed[0]
    ones = torch.ones(1, dim, device=DEV)
    out = ops.csr_mean(gr.rp_d, gr.col_d, ones, self_loop=True, index=torch.zeros(n, dtype=torch.int32, device=DEV))
    assert gr.own[8] and not gr.own[4]
    for v in (4, 8):
        c = int(gr.deg[v]) + (0 if gr.own[v] else 1)
        assert float(out[v, 0]) == float(np.float32(c) * (np.float32(1.0) / np.float32(c)))
    with pytest.raises(native.SageError):
        ops.csr_mean(gr.rp_d, gr.col_d, embed, index=raw[:-1])                       # len(index) != N
    with pytest.raises(native.SageError):
        ops.csr_mean(gr.rp_d, gr.col_d, embed, index=raw.long())                     # not int32


# ----------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("dim,pad", [(64, 0), (50, 0), (64, 4), (50, 3)])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("kind", ["identity", "degree", "zero"])
def test_grouped_backward_against_fp64(graphs, kind, self_loop, dim, pad):
    gr = graphs["sym"]
    g, g_dev = _grad(gr.n, dim, pad, seed=dim + pad)
    got = gr.run(g_dev, kind, self_loop)
    want, A = gr.reference(g, kind, self_loop)
    assert tuple(got.shape) == tuple(want.shape)
    _check(got, want, A, f"{kind} dim={dim} ldg={dim + pad} self_loop={self_loop}")


@pytest.mark.parametrize("name", ["sym", "rev"])
def test_grouped_backward_with_the_identity_index_is_csr_mean_backward_bit_for_bit(graphs, name):
    """Without self entries the grouped rows ARE the transposed rows: the same sequences, the same chunks."""
    gr = graphs[name]
    rp_t, c_t = ops.csr_transpose(gr.rp_d, gr.col_d)
    grouped = gr.grouped("identity", False)
    assert torch.equal(grouped.rowptr, rp_t) and torch.equal(grouped.col, c_t)
    if name == "rev":
        assert {0, 1, E - 1, E, E + 1, 2 * E, 2 * E + 1, 20 * E + 37} <= set(torch.diff(rp_t).tolist())
    for dim, pad in ((64, 0), (50, 3)):
        _, g_dev = _grad(gr.n, dim, pad, seed=7)
        want = ops.csr_mean_backward(gr.rp_d, gr.col_d, rp_t, c_t, g_dev, self_loop=False)
        assert bits_equal(gr.run(g_dev, "identity", False), want), (name, dim, pad)


@pytest.mark.parametrize("kind", ["degree", "zero"])
def test_grouped_backward_bits_and_what_it_writes(graphs, kind):
    """Two runs, a max_edges below the truth (no room, room for some chunks, room for all but the hub) and a garbage workspace
    change no bit; rows of `out` past K and columns past dim are not written."""
    gr = graphs["sym"]
    for dim, pad in ((64, 4), (50, 3)):
        _, g_dev = _grad(gr.n, dim, 0, seed=11)
        for self_loop in (False, True):
            k = gr.grouped(kind, self_loop).rowptr.shape[0] - 1
            full = gr.run(g_dev, kind, self_loop)
            assert bits_equal(gr.run(g_dev, kind, self_loop), full), "two calls differ"
            for max_edges in (0, 3 * E, 25 * E):
                assert bits_equal(gr.run(g_dev, kind, self_loop, max_edges=max_edges), full), (dim, self_loop, max_edges)
            need = ops.csr_mean_backward_grouped_workspace_bytes(gr.n, k, gr.grouped(kind, self_loop).col.numel(), dim)
            ws = torch.randint(0, 256, (need,), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
            big = torch.full((k + 5, dim + pad), SENTINEL, device=DEV)
            big[:k, :dim] = torch.randn(k, dim, device=DEV) * 1e30
            gr.run(g_dev, kind, self_loop, out=big[:, :dim], workspace=ws)
            assert bits_equal(big[:k, :dim], full), "a prefilled output / workspace changed the result"
            assert bool((big[:, dim:] == SENTINEL).all()) and bool((big[k:] == SENTINEL).all()), "padding columns or rows past K written"


def test_grouped_backward_refuses_a_list_of_another_kind(graphs):
    gr = graphs["sym"]
    _, g_dev = _grad(gr.n, 8, 0, seed=1)
    g = gr.grouped("degree", True)
    with pytest.raises(native.SageError):
        ops.csr_mean_backward_grouped(gr.rp_d, gr.col_d, (g.rowptr, g.col), g_dev)     # the flag must travel with the list
    with pytest.raises(native.SageError):
        ops.csr_mean_backward_grouped(gr.rp_d, gr.col_d, g, g_dev[:-1])
    with pytest.raises(TypeError):
        ops.csr_mean_backward_grouped(gr.rp_d, gr.col_d, g, g_dev, self_loop=False)    # no such argument


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("kind", ["degree", "zero"])
def test_grouped_backward_is_the_adjoint_of_the_indexed_forward(graphs, kind, self_loop):
    """<csr_mean(embed, index), G> == <embed, backward_grouped(G)> in fp64 within the bound."""
    gr = graphs["sym"]
    dim = 64
    ix, k = gr.index_dev(kind)
    x = torch.randn(k, dim, generator=torch.Generator().manual_seed(2))
    g, g_dev = _grad(gr.n, dim, 0, seed=3)
    fwd = ops.csr_mean(gr.rp_d, gr.col_d, x.to(DEV), self_loop=self_loop, index=ix).double().cpu()
    bwd = gr.run(g_dev, kind, self_loop).double().cpu()
    lhs, rhs = float((fwd * g.double()).sum()), float((x.double() * bwd).sum())
    want, A = gr.reference(g, kind, self_loop)
    bound = BOUND * float((x.double().abs() * A).sum())
    print(f"<F(X), G> = {lhs}, <X, B(G)> = {rhs}, bound {bound:.3g}")
    assert abs(lhs - rhs) <= bound, f"<F(X), G> = {lhs}, <X, B(G)> = {rhs}: differ by {abs(lhs - rhs):.3g} > {bound:.3g}"
    _check(bwd, want, A, "adjoint case")


@pytest.mark.parametrize("dim", [50, 64])
@pytest.mark.parametrize("kind", ["degree", "zero"])
def test_autograd_csr_mean_with_an_index_matches_fp64_autograd(graphs, kind, dim):
    """Against stock fp64 autograd of embed[index] averaged by index_add_ on the CPU, with the forward's own float weights."""
    gr = graphs["sym"]
    ix, k = gr.index_dev(kind)
    ix64 = torch.from_numpy(gr.index(kind)[0])
    src, dst = torch.from_numpy(gr.src), torch.from_numpy(gr.col.astype(np.int64))
    g, g_dev = _grad(gr.n, dim, 0, seed=13)
    for self_loop in (False, True):
        embed = torch.randn(k, dim, device=DEV, requires_grad=True)
        out = autograd.csr_mean(gr.rp_d, gr.col_d, embed, self_loop=self_loop, index=ix, grouped=gr.grouped(kind, self_loop))
        assert bits_equal(out.detach(), ops.csr_mean(gr.rp_d, gr.col_d, embed.detach()[ix.long()], self_loop=self_loop))
        out.backward(g_dev)
        extra, w = gr.weights(self_loop)
        e64 = embed.detach().double().cpu().requires_grad_(True)
        x = e64[ix64]
        ref = torch.zeros(gr.n, dim, dtype=torch.float64).index_add(0, src, x[dst])
        ref = (ref + x * torch.from_numpy(extra).double()[:, None]) * w[:, None]
        assert float((out.detach().double().cpu() - ref.detach()).abs().max()) <= 1e-5 * float(ref.detach().abs().max())
        ref.backward(g.double())
        _, A = gr.reference(g, kind, self_loop)
        _check(embed.grad, e64.grad, A, f"autograd {kind} dim={dim} self_loop={self_loop}")
        e2 = embed.detach().clone().requires_grad_(True)                          # the list built by the wrapper: the same bits
        autograd.csr_mean(gr.rp_d, gr.col_d, e2, self_loop=self_loop, index=ix).backward(g_dev)
        assert bits_equal(e2.grad, embed.grad)
    with pytest.raises(native.SageError):                                        # a list built with the other flag
        autograd.csr_mean(gr.rp_d, gr.col_d, embed, self_loop=False, index=ix, grouped=gr.grouped(kind, True))
    with torch.no_grad():
        assert bits_equal(autograd.csr_mean(gr.rp_d, gr.col_d, embed, index=ix), ops.csr_mean(gr.rp_d, gr.col_d, embed.detach(), index=ix))
