"""sage_csr_mean_backward (the adjoint of the full-neighbourhood mean, include/sage355.h) on the MI355X: against an fp64
reference built on the CPU from the documented formula, as the adjoint of ops.csr_mean, bitwise reproducibility, what is not
written and not read, and the autograd wrapper.

Graphs.  "sym": the edge list of the skewed graph of tests/test_gpu_csr_mean.py (generator copied below) together with its reverse,
n = 24 * 512 nodes -- forward and transposed rows both hold a hub of more than 20 E entries, rows of one and of several chunks,
self-loop entries (one in the last chunk of a long row), unsorted rows, duplicates and rows without entries.  Adding the
reverse moves the exact row lengths (every node gains its in-degree), so two directed graphs pin them: "fwd" is the skewed graph
itself (FORWARD rows of exactly 0, 1, E-1, E, E+1, 2E, 2E+1 and 20E+37 entries: the self scan and the weights), "rev" its
transpose (TRANSPOSED rows of exactly those lengths: the chunked sum).

Tolerance (tests/test_gpu_backward_kernels.py): |got - want| <= 1e-5 * A elementwise, A the fp64 sum of the terms' absolute
values; exact zeros where A = 0; max |err| / max |want| <= 2e-5."""
import numpy as np
import pytest
import torch

from sage355 import autograd, native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = native.CSR_MEAN_CHUNK
BOUND, MAXREL = 1e-5, 2e-5
SENTINEL = -31.5


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def skewed_graph(seed=0):
    """Rows of degree 0, 1, E-1, E, E+1, 2E, 2E+1 and one star hub of 20E + 37, among rows of 0..6 edges; some rows hold
    their own node (a self-loop edge), neighbour lists unsorted."""
    rng = np.random.default_rng(seed)
    n = 24 * E
    special = {0: 0, 1: 1, 2: E - 1, 3: E, 4: E + 1, 5: 2 * E, 6: 2 * E + 1, 7: 20 * E + 37, 8: E + 1, 9: 2 * E + 1}
    deg = rng.integers(0, 7, n)
    for v, d in special.items():
        deg[v] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    col[rowptr[7]:rowptr[8]] = rng.permutation(n)[: deg[7]]          # the hub: a star over distinct nodes
    for v in (3, 8, 9, 20, 21, 22):                                     # self-loop edges (rows 8, 9 in their last chunk)
        if deg[v] > 0:
            col[rowptr[v + 1] - 1] = v
    col[rowptr[7] + 5 * E + 3] = 7
    return rowptr, col


class Graph:
    """A forward CSR, its transpose (ops.csr_transpose on the CPU) and the fp64 ingredients of the formula."""

    def __init__(self, rowptr, col):
        self.rowptr, self.col = rowptr, col
        self.n = len(rowptr) - 1
        self.deg = np.diff(rowptr)
        self.src = np.repeat(np.arange(self.n), self.deg)
        rp_t, c_t = ops.csr_transpose(torch.from_numpy(rowptr), torch.from_numpy(col))
        self.deg_t = np.diff(rp_t.numpy())
        self.own = np.zeros(self.n, dtype=bool)                         # v is an entry of its own row
        self.own[self.src[col == self.src]] = True
        self.dev = tuple(t.to(DEV) for t in (torch.from_numpy(rowptr), torch.from_numpy(col), rp_t, c_t))
        self._ref = {}

    def weights(self, self_loop):
        extra = (~self.own) if self_loop else np.zeros(self.n, dtype=bool)
        c = self.deg + extra
        w = np.zeros(self.n, dtype=np.float32)
        w[c > 0] = np.float32(1.0) / c[c > 0].astype(np.float32)        # the forward's own float
        return extra, torch.from_numpy(w.astype(np.float64))

    def reference(self, g, self_loop):
        """(want, A) fp64 [n, dim]: index_add_ over the forward's edges (v -> u): w_v g_v onto row u, plus the self term."""
        extra, w = self.weights(self_loop)
        g64 = g.double()
        term = g64 * w[:, None]
        src, dst = torch.from_numpy(self.src), torch.from_numpy(self.col.astype(np.int64))
        want = torch.zeros_like(g64).index_add_(0, dst, term[src])
        A = torch.zeros_like(g64).index_add_(0, dst, term[src].abs())
        ex = torch.from_numpy(extra)
        want[ex] += term[ex]
        A[ex] += term[ex].abs()
        return want, A

    def run(self, g, self_loop, **kw):
        return ops.csr_mean_backward(*self.dev, g, self_loop=self_loop, **kw)


def _sym():
    rowptr, col = skewed_graph()
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n), np.diff(rowptr))
    s = np.concatenate([src, col.astype(np.int64)])
    d = np.concatenate([col.astype(np.int64), src])
    order = np.argsort(s, kind="stable")                                # a row: its own entries as they were, then the reversed ones
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(s, minlength=n), out=rp[1:])
    return Graph(rp, d[order].astype(np.int32))


def _rev():
    rowptr, col = skewed_graph()
    rp_t, c_t = ops.csr_transpose(torch.from_numpy(rowptr), torch.from_numpy(col))
    return Graph(rp_t.numpy(), c_t.numpy())


@pytest.fixture(scope="module")
def graphs():
    gs = {"sym": _sym(), "fwd": Graph(*skewed_graph()), "rev": _rev()}
    lengths = {0, 1, E - 1, E, E + 1, 2 * E, 2 * E + 1, 20 * E + 37}
    assert lengths <= set(gs["fwd"].deg.tolist()) and lengths <= set(gs["rev"].deg_t.tolist())
    s = gs["sym"]
    assert s.n == 24 * E and s.deg.max() > 20 * E and s.deg_t.max() > 20 * E and np.array_equal(s.deg, s.deg_t)
    assert ((s.deg > E) & (s.deg <= 2 * E)).any() and (s.deg > 2 * E).sum() >= 3 and (s.deg == 0).any() and s.own.any()
    assert s.own[8] and s.own[9] and s.deg[9] > 2 * E                   # a self-loop entry beyond the first chunks of a long row
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


CASES = [("sym", d, p) for d, p in [(1, 0), (3, 0), (4, 0), (50, 3), (128, 0), (128, 4)]] + \
        [(name, d, p) for name in ("fwd", "rev") for d, p in [(3, 0), (128, 4)]]


@pytest.mark.parametrize("name,dim,pad", CASES)
@pytest.mark.parametrize("self_loop", [False, True])
def test_csr_mean_backward_against_fp64(graphs, name, dim, pad, self_loop):
    gr = graphs[name]
    g, g_dev = _grad(gr.n, dim, pad, seed=dim + pad)
    got = gr.run(g_dev, self_loop)
    want, A = gr.reference(g, self_loop)
    _check(got, want, A, f"{name} dim={dim} ldg={dim + pad} self_loop={self_loop}")


@pytest.mark.parametrize("self_loop", [False, True])
def test_csr_mean_backward_is_the_adjoint_of_the_forward(graphs, self_loop):
    """<csr_mean(X), G> == <X, csr_mean_backward(G)> in fp64 within the bound."""
    gr = graphs["sym"]
    dim = 64
    x = torch.randn(gr.n, dim, generator=torch.Generator().manual_seed(2))
    g, g_dev = _grad(gr.n, dim, 0, seed=3)
    fwd = ops.csr_mean(gr.dev[0], gr.dev[1], x.to(DEV), self_loop=self_loop).double().cpu()
    bwd = gr.run(g_dev, self_loop).double().cpu()
    lhs, rhs = float((fwd * g.double()).sum()), float((x.double() * bwd).sum())
    want, A = gr.reference(g, self_loop)
    bound = BOUND * float((x.double().abs() * A).sum())
    print(f"<F(X), G> = {lhs}, <X, B(G)> = {rhs}, bound {bound:.3g}")
    assert abs(lhs - rhs) <= bound, f"<F(X), G> = {lhs}, <X, B(G)> = {rhs}: differ by {abs(lhs - rhs):.3g} > {bound:.3g}"
    _check(bwd, want, A, "adjoint case")


@pytest.mark.parametrize("name", ["sym", "rev"])
def test_csr_mean_backward_bits(graphs, name):
    """Two calls, a row subset (the first ten rows, the hub twice, 200 random rows, duplicates) against the full result, and a
    max_edges below the truth (no room, room for some chunks, room for all) against the default: the same bits."""
    gr = graphs[name]
    hub = int(np.argmax(gr.deg_t))
    rng = np.random.default_rng(5)
    subset = np.concatenate([np.arange(10), [hub, hub, 5, 0], rng.integers(0, gr.n, 200), [21, 9, 9]]).astype(np.int64)
    for dim, pad in ((64, 0), (50, 3)):
        _, g_dev = _grad(gr.n, dim, pad, seed=7)
        for self_loop in (False, True):
            full = gr.run(g_dev, self_loop)
            assert bits_equal(gr.run(g_dev, self_loop), full), "two calls differ"
            sub = gr.run(g_dev, self_loop, nodes=torch.from_numpy(subset.astype(np.int32)).to(DEV))
            assert bits_equal(sub, full[torch.from_numpy(subset).to(DEV)]), "backward(nodes=S) != backward()[S] bitwise"
            for max_edges in (0, 3 * E, 25 * E):
                assert bits_equal(gr.run(g_dev, self_loop, max_edges=max_edges), full), (dim, self_loop, max_edges)


@pytest.mark.parametrize("dim,pad", [(64, 4), (50, 3)])
def test_csr_mean_backward_writes_and_reads_only_what_it_says(graphs, dim, pad):
    gr = graphs["sym"]
    n = gr.n
    _, g_dev = _grad(n, dim, 0, seed=11)
    need = ops.csr_mean_backward_workspace_bytes(n, n, gr.col.size, dim)
    for self_loop in (False, True):
        ref = gr.run(g_dev, self_loop)
        # columns [dim, ldgt) and rows past n keep a sentinel; a garbage prefill of grad_table and of the workspace changes nothing
        big = torch.full((n + 5, dim + pad), SENTINEL, device=DEV)
        big[:n, :dim] = torch.randn(n, dim, device=DEV) * 1e30
        ws = torch.randint(0, 256, (need,), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        gr.run(g_dev, self_loop, out=big[:, :dim], workspace=ws)
        assert bits_equal(big[:n, :dim], ref), f"self_loop={self_loop}: prefilled output / workspace changed the result"
        assert bool((big[:, dim:] == SENTINEL).all()) and bool((big[n:] == SENTINEL).all()), "padding columns or rows past n written"
        ws.fill_(255)
        assert bits_equal(gr.run(g_dev, self_loop, workspace=ws), ref)
        sub = torch.full((40, dim + pad), SENTINEL, device=DEV)
        gr.run(g_dev, self_loop, nodes=torch.arange(30, dtype=torch.int32, device=DEV), out=sub[:, :dim])
        assert bits_equal(sub[:30, :dim], ref[:30]) and bool((sub[30:] == SENTINEL).all()) and bool((sub[:, dim:] == SENTINEL).all())
    # rows of grad_out that belong to no term are not read: nodes without entries, when no self term is added
    empty = torch.from_numpy(np.nonzero(gr.deg == 0)[0]).to(DEV)
    assert empty.numel() > 0
    poisoned = g_dev.clone()
    poisoned[empty] = float("nan")
    assert bits_equal(gr.run(poisoned, False), gr.run(g_dev, False)), "NaN in an unused grad_out row reached the result"


@pytest.mark.parametrize("dim", [50, 128])
def test_autograd_csr_mean_backward_matches_fp64(graphs, dim):
    gr = graphs["sym"]
    rp, cl, rp_t, c_t = gr.dev
    g, g_dev = _grad(gr.n, dim, 0, seed=13)
    for self_loop in (False, True):
        table = torch.randn(gr.n + 3, dim, device=DEV, requires_grad=True)        # three rows past the graph
        out = autograd.csr_mean(rp, cl, table, transpose=(rp_t, c_t), self_loop=self_loop)
        assert bits_equal(out.detach(), ops.csr_mean(rp, cl, table.detach(), self_loop=self_loop))
        out.backward(g_dev)
        want, A = gr.reference(g, self_loop)
        _check(table.grad[:gr.n], want, A, f"autograd dim={dim} self_loop={self_loop}")
        assert bool((table.grad[gr.n:] == 0).all()), "table rows past num_nodes must get a zero gradient"
        t2 = table.detach().clone().requires_grad_(True)                          # the transpose built by the wrapper: the same bits
        autograd.csr_mean(rp, cl, t2, self_loop=self_loop).backward(g_dev)
        assert bits_equal(t2.grad, table.grad)


def test_autograd_csr_mean_refuses_a_row_subset_and_passes_through_without_grad(graphs):
    gr = graphs["sym"]
    rp, cl = gr.dev[:2]
    table = torch.randn(gr.n, 8, device=DEV, requires_grad=True)
    nodes = torch.arange(5, dtype=torch.int32, device=DEV)
    with pytest.raises(native.SageError):
        autograd.csr_mean(rp, cl, table, nodes=nodes)
    with torch.no_grad():
        out = autograd.csr_mean(rp, cl, table, nodes=nodes)
    assert not out.requires_grad and bits_equal(out, ops.csr_mean(rp, cl, table.detach(), nodes=nodes))
    out = autograd.csr_mean(rp, cl, table.detach())
    assert not out.requires_grad and bits_equal(out, ops.csr_mean(rp, cl, table.detach()))
