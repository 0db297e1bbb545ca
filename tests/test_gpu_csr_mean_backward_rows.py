"""sage_csr_mean_backward_rows (the adjoint of the indexed full-neighbourhood mean of a SEED BATCH, include/sage355.h) on the MI355X.

The graph (6000 nodes) and the batch (2095 seed rows, shuffled) are built so that, without the set-union self term, frontier rows
receive exactly 0, 1, 63, 64, 65, 511, 512, 513, 1025 and 1537 terms: filler seed i names target t_c exactly when i < c.  The batch
also holds a seed whose own row has 1537 entries (three chunks of term positions from one row), one seed twice, a row that names the
same neighbour twice, two seeds that are entries of their own rows, seeds with empty rows and one id outside the graph.

1. bit for bit against sage_csr_mean_backward_grouped fed the sorted term list built on the host (numpy stable sort) and a surrogate
   forward CSR over the seed rows: the same fmas in the same order through the same chunk rule.  This pins the term order.
2. against fp64: |got - want| <= 1e-5 * A elementwise (A the fp64 sum of the terms' absolute values), exact zeros where A = 0,
   max |err| / max |want| <= 2e-5 -- the constants of tests/test_gpu_csr_mean_backward.py, whose kernel does this arithmetic -- and
   the adjoint identity with the forward within the same bound.
3. the bits depend on neither the placement of the rows nor the run; 4. they are sage_csr_mean_backward's where that applies;
5. a max_edges below the truth drops terms, reports the true count and writes nothing out of range; 6. the autograd wrapper."""
import numpy as np
import pytest
import torch

from sage355 import autograd, native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = native.CSR_MEAN_CHUNK
BOUND, MAXREL = 1e-5, 2e-5
SENTINEL = -31.5
COUNTS = (0, 1, 63, 64, 65, 511, 512, 513, 1025, 1537)
N = 6000
CASES = [(d, p) for d in (1, 3, 4, 12, 260) for p in (0, 4)] + [(12, 3)]


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def build_graph():
    rng = np.random.default_rng(0)
    role = rng.permutation(N)
    k = len(COUNTS) - 1
    targets = {c: int(role[i]) for i, c in enumerate(COUNTS[1:])}
    fill = role[k:k + 1537]
    hub, dup, twice, self_a, self_b, lonely = (int(x) for x in role[k + 1537:k + 1543])
    more = role[k + 1543:k + 2093]
    pool = role[k + 2093:]                                         # ordinary neighbours: named by whoever draws them
    rows = {int(v): list(rng.integers(0, N, rng.integers(0, 6))) for v in role}          # nodes that are no seeds: never read
    for i, s in enumerate(fill):
        row = [targets[c] for c in COUNTS[1:] if i < c] + list(rng.choice(pool, rng.integers(0, 4)))
        rows[int(s)] = list(rng.permutation(row))
    rows[hub] = list(rng.choice(pool, 1537, replace=False))
    rows[dup] = list(rng.choice(pool, 5, replace=False))
    p, q = (int(x) for x in rng.choice(pool, 2, replace=False))
    rows[twice] = [p, q, p]
    rows[self_a] = [int(pool[0]), self_a, int(pool[1])]
    rows[self_b] = [self_b]
    rows[lonely] = [int(pool[2])]
    for s in more:
        rows[int(s)] = list(rng.choice(pool, rng.integers(0, 7)))  # some of them empty
    deg = np.array([len(rows[v]) for v in range(N)])
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([np.asarray(rows[v], dtype=np.int32) for v in range(N)])
    batch = np.concatenate([fill, [hub, dup, dup, twice, self_a, self_b, lonely], more, [N + 7]]).astype(np.int32)
    batch = batch[rng.permutation(len(batch))]
    return rowptr, col, batch, dict(targets=targets, hub=hub, dup=dup, twice=twice, self_a=self_a, self_b=self_b, lonely=lonely)


def host_terms(rowptr, col, nodes, self_loop):
    """The batch's terms in the documented order -> (node id of every term, seed row of every term, w [m] fp32) and the surrogate
    forward CSR over the seed rows (row r holds r exactly where the original row holds nodes[r])."""
    m = len(nodes)
    ids, vals, srows = [], [], []
    w = np.zeros(m, dtype=np.float32)
    sdeg = np.zeros(m, dtype=np.int64)
    for r, v in enumerate(nodes.tolist()):
        if v < 0 or v >= N:
            continue                                              # an empty row without a self term
        row = col[rowptr[v]:rowptr[v + 1]]
        extra = bool(self_loop) and not bool((row == v).any())
        c = len(row) + int(extra)
        if c > 0:
            w[r] = np.float32(1.0) / np.float32(c)                # the forward's own float
        ids.append(row)
        vals.append(np.full(len(row), r, dtype=np.int32))
        if extra:
            ids.append(np.array([v], dtype=np.int32))
            vals.append(np.array([r], dtype=np.int32))
        srows.append(np.where(row == v, r, (r + 1) % m).astype(np.int32))
        sdeg[r] = len(row)
    srp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(sdeg, out=srp[1:])
    return np.concatenate(ids), np.concatenate(vals), w, srp, np.concatenate(srows)


class Batch:
    def __init__(self):
        self.rowptr, self.col, self.nodes, self.who = build_graph()
        self.m = len(self.nodes)
        self.dev = tuple(torch.from_numpy(x).to(DEV) for x in (self.rowptr, self.col, self.nodes))
        fr = ops.CsrFrontier(N, DEV)
        ops.csr_frontier(self.dev[0], self.dev[1], self.dev[2], fr)
        self.rows = fr.size()
        self.pos = fr.pos.clone()
        self.f_nodes = fr.nodes[:self.rows].clone()
        self.pos_host = self.pos.cpu().numpy()
        self.host = {}
        for self_loop in (False, True):
            ids, vals, w, srp, scol = host_terms(self.rowptr, self.col, self.nodes, self_loop)
            keys = self.pos_host[ids]
            assert keys.min() >= 0 and keys.max() < self.rows
            order = np.argsort(keys, kind="stable")
            rowptr_f = np.zeros(self.rows + 1, dtype=np.int64)
            np.cumsum(np.bincount(keys, minlength=self.rows), out=rowptr_f[1:])
            self.host[self_loop] = dict(keys=keys, vals=vals, w=w, rowptr_f=rowptr_f, vals_sorted=vals[order].astype(np.int32),
                                        srp=torch.from_numpy(srp).to(DEV), scol=torch.from_numpy(scol).to(DEV))

    def run(self, g_dev, self_loop, **kw):
        kw.setdefault("index", self.pos)
        kw.setdefault("num_rows", self.rows)
        return ops.csr_mean_backward_rows(self.dev[0], self.dev[1], self.dev[2], g_dev, self_loop=self_loop, **kw)

    def grouped(self, g_dev, self_loop, out=None):
        """The parent's kernel on the host-built list: the same fmas in the same order through the same chunk rule."""
        h = self.host[self_loop]
        gt = ops.GroupedTranspose(torch.from_numpy(h["rowptr_f"]).to(DEV), torch.from_numpy(h["vals_sorted"]).to(DEV), self_loop)
        return ops.csr_mean_backward_grouped(h["srp"], h["scol"], gt, g_dev, out=out)

    def reference(self, g, self_loop):
        """(want, A) fp64 [rows, dim] from the fp32 inputs with the fp32 weight."""
        h = self.host[self_loop]
        term = g.double().numpy()[h["vals"]] * h["w"].astype(np.float64)[h["vals"], None]
        want = np.zeros((self.rows, g.shape[1]))
        A = np.zeros_like(want)
        np.add.at(want, h["keys"], term)
        np.add.at(A, h["keys"], np.abs(term))
        return torch.from_numpy(want), torch.from_numpy(A)


@pytest.fixture(scope="module")
def batch():
    b = Batch()
    assert 2050 <= b.m <= 2150
    per_row = np.diff(b.host[False]["rowptr_f"])
    for c, t in b.who["targets"].items():
        assert per_row[b.pos_host[t]] == c, (c, per_row[b.pos_host[t]])
    assert per_row[b.pos_host[b.who["lonely"]]] == 0 and set(COUNTS) <= set(per_row.tolist())
    deg = np.diff(b.rowptr)
    assert deg[b.who["hub"]] == 1537 and (b.nodes == b.who["dup"]).sum() == 2 and (b.nodes >= N).sum() == 1
    assert (deg[b.nodes[b.nodes < N]] == 0).any() and b.pos_host[b.who["self_a"]] >= 0
    assert len(b.host[True]["keys"]) > len(b.host[False]["keys"]) > b.m
    return b


def _grad(n, dim, pad, seed):
    """grad_out [n, dim] on the CPU and its device copy with leading dimension dim + pad (the padding holds the sentinel)."""
    g = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))
    wide = torch.full((n, dim + pad), SENTINEL)
    wide[:, :dim] = g
    return g, (wide.to(DEV)[:, :dim] if pad else wide.to(DEV))


def _padded_out(rows, dim, pad, guard=3):
    big = torch.full((rows + 2 * guard, dim + pad), SENTINEL, device=DEV)
    return big, big[guard:guard + rows, :dim]


def _untouched(big, rows, dim, guard=3):
    return bool((big[:guard] == SENTINEL).all()) and bool((big[guard + rows:] == SENTINEL).all()) and bool((big[:, dim:] == SENTINEL).all())


@pytest.mark.parametrize("dim,pad", CASES)
@pytest.mark.parametrize("self_loop", [False, True])
def test_bit_exact_against_the_grouped_kernel_on_the_host_sorted_list(batch, dim, pad, self_loop):
    _, g_dev = _grad(batch.m, dim, pad, seed=dim + pad)
    big, out = _padded_out(batch.rows, dim, pad)
    got = batch.run(g_dev, self_loop, out=out)
    assert _untouched(big, batch.rows, dim), "padding columns or guard rows written"
    big2, out2 = _padded_out(batch.rows, dim, pad)
    want = batch.grouped(g_dev, self_loop, out=out2)
    diff = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    print(f"dim={dim} pad={pad} self_loop={self_loop}: {diff} of {got.numel()} elements differ from the grouped kernel")
    assert diff == 0, f"{diff} elements differ from csr_mean_backward_grouped on the documented term order"


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


@pytest.mark.parametrize("dim,pad", CASES)
@pytest.mark.parametrize("self_loop", [False, True])
def test_against_fp64(batch, dim, pad, self_loop):
    g, g_dev = _grad(batch.m, dim, pad, seed=100 + dim + pad)
    big, out = _padded_out(batch.rows, dim, pad)
    got = batch.run(g_dev, self_loop, out=out)
    want, A = batch.reference(g, self_loop)
    _check(got, want, A, f"dim={dim} ldg={dim + pad} self_loop={self_loop}")
    assert _untouched(big, batch.rows, dim)


@pytest.mark.parametrize("self_loop", [False, True])
def test_it_is_the_adjoint_of_the_indexed_forward(batch, self_loop):
    """<csr_mean(X, nodes, index), G> == <X, backward_rows(G)> in fp64 within the bound."""
    dim = 64
    x = torch.randn(batch.rows, dim, generator=torch.Generator().manual_seed(2))
    g, g_dev = _grad(batch.m, dim, 0, seed=3)
    rp, cl, nodes = batch.dev
    fwd = ops.csr_mean(rp, cl, x.to(DEV), nodes=nodes, self_loop=self_loop, index=batch.pos).double().cpu()
    bwd = batch.run(g_dev, self_loop).double().cpu()
    lhs, rhs = float((fwd * g.double()).sum()), float((x.double() * bwd).sum())
    want, A = batch.reference(g, self_loop)
    bound = BOUND * float((x.double().abs() * A).sum())
    print(f"<F(X), G> = {lhs}, <X, B(G)> = {rhs}, bound {bound:.3g}")
    assert abs(lhs - rhs) <= bound, f"<F(X), G> = {lhs}, <X, B(G)> = {rhs}: differ by {abs(lhs - rhs):.3g} > {bound:.3g}"
    _check(bwd, want, A, "adjoint case")


@pytest.mark.parametrize("dim,pad", [(12, 0), (50, 3), (260, 4)])
def test_the_bits_depend_on_neither_placement_nor_run(batch, dim, pad):
    _, g_dev = _grad(batch.m, dim, pad, seed=7)
    rp, cl, nodes = batch.dev
    perm = torch.from_numpy(np.random.default_rng(1).permutation(batch.rows)).to(DEV)
    pos2 = torch.where(batch.pos >= 0, perm[batch.pos.long().clamp_min(0)].to(torch.int32), batch.pos)
    ident = torch.arange(N, dtype=torch.int32, device=DEV)
    for self_loop in (False, True):
        got = batch.run(g_dev, self_loop)
        assert bits_equal(batch.run(g_dev, self_loop), got), "two calls differ"
        moved = batch.run(g_dev, self_loop, index=pos2)
        assert bits_equal(moved[perm], got), "a permuted map changed the bits of a node's row"
        by_node = ops.csr_mean_backward_rows(rp, cl, nodes, g_dev, self_loop=self_loop)
        assert by_node.shape == (N, dim)
        assert bits_equal(by_node, batch.run(g_dev, self_loop, index=ident, num_rows=N)), "index=None is not the identity map"
        assert bits_equal(by_node[batch.f_nodes.long()], got), "a node's row differs between the identity map and the frontier's"
        outside = torch.ones(N, dtype=torch.bool, device=DEV)
        outside[batch.f_nodes.long()] = False
        assert bool((by_node[outside] == 0).all()), "a row nobody read is not zeros"
        nan = torch.full((batch.rows, dim), float("nan"), device=DEV)
        need = ops.csr_mean_backward_rows_workspace_bytes(batch.m, int(batch.rowptr[-1]), batch.rows, dim)
        ws = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
        filled = batch.run(g_dev, self_loop, out=nan, workspace=ws)
        assert not bool(torch.isnan(filled).any()) and bits_equal(filled, got), "grad_table is stored, not accumulated"


@pytest.mark.parametrize("dim", [3, 64])
def test_bit_equal_to_csr_mean_backward_where_the_orders_coincide(dim):
    """self_loop off, ascending distinct seeds, in-degrees at or below the chunk: the transpose lists a row's sources in ascending
    order, which is the batch's row order, and the sources outside the batch add fma(w, 0, acc) = acc."""
    rng = np.random.default_rng(4)
    n = 3000
    deg = rng.integers(0, 9, n)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    assert np.bincount(col, minlength=n).max() <= E
    seeds = np.sort(rng.choice(n, 700, replace=False)).astype(np.int32)
    rp, cl, sd = (torch.from_numpy(x).to(DEV) for x in (rowptr, col, seeds))
    rp_t, c_t = ops.csr_transpose(rp, cl)
    fr = ops.CsrFrontier(n, DEV)
    ops.csr_frontier(rp, cl, sd, fr)
    f_nodes = fr.nodes[:fr.size()]
    g = torch.randn(len(seeds), dim, device=DEV)
    scattered = torch.zeros(n, dim, device=DEV).index_copy_(0, sd.long(), g)
    want = ops.csr_mean_backward(rp, cl, rp_t, c_t, scattered, nodes=f_nodes)
    got = ops.csr_mean_backward_rows(rp, cl, sd, g, index=fr.pos, num_rows=f_nodes.shape[0])
    assert bits_equal(got, want)


@pytest.mark.parametrize("self_loop", [False, True])
def test_a_max_edges_below_the_truth_drops_terms_reports_the_count_and_stays_in_range(batch, self_loop):
    dim = 12
    _, g_dev = _grad(batch.m, dim, 0, seed=9)
    h = batch.host[self_loop]
    entries = int(sum(batch.rowptr[v + 1] - batch.rowptr[v] for v in batch.nodes.tolist() if 0 <= v < N))
    total = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    full = batch.run(g_dev, self_loop, max_edges=entries, total_terms=total)
    assert int(total) == len(h["keys"])
    assert bits_equal(full, batch.run(g_dev, self_loop)), "the exact bound and the host-read default differ"
    big, out = _padded_out(batch.rows, dim, 4)
    total.fill_(-1)
    short = batch.run(g_dev, self_loop, out=out, max_edges=entries - 1, total_terms=total)
    assert int(total) == len(h["keys"]), "total_terms must report the true count"
    assert _untouched(big, batch.rows, dim), "something outside grad_table's [num_rows, dim] was written"
    assert not bool(torch.isnan(short).any())
    # without the self terms the capacity is one short: the last term is dropped and its row alone changes.  With them the capacity
    # counts a self term for every seed row, more than the batch has (two seeds are their own entries, one id is outside the graph)
    last = int(h["keys"][-1])
    keep = torch.ones(batch.rows, dtype=torch.bool, device=DEV)
    keep[last] = False
    assert bits_equal(short[keep], full[keep])
    assert bits_equal(short[last], full[last]) == bool(self_loop)
    # no seed rows: zeros in every row
    none = torch.full((batch.rows, dim), float("nan"), device=DEV)
    rp, cl, _ = batch.dev
    total.fill_(-1)
    ops.csr_mean_backward_rows(rp, cl, torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dim, device=DEV), index=batch.pos,
                               num_rows=batch.rows, self_loop=self_loop, out=none, total_terms=total)
    assert bool((none == 0).all()) and int(total) == 0


@pytest.mark.parametrize("dim", [12, 50])
def test_autograd_csr_mean_rows(batch, dim):
    rp, cl, nodes = batch.dev
    _, g_dev = _grad(batch.m, dim, 0, seed=13)
    for self_loop in (False, True):
        table = torch.randn(batch.rows, dim, device=DEV, requires_grad=True)
        out = autograd.csr_mean_rows(rp, cl, table, nodes, index=batch.pos, self_loop=self_loop)
        assert out.requires_grad and bits_equal(out.detach(), ops.csr_mean(rp, cl, table.detach(), nodes=nodes, self_loop=self_loop, index=batch.pos))
        out.backward(g_dev)
        assert bits_equal(table.grad, batch.run(g_dev, self_loop)), "backward() does not give the operator's bits"
        wide = torch.randn(N + 3, dim, device=DEV, requires_grad=True)           # no index: by node id, three rows past the graph
        autograd.csr_mean_rows(rp, cl, wide, nodes, self_loop=self_loop).backward(g_dev)
        assert bits_equal(wide.grad[:N], ops.csr_mean_backward_rows(rp, cl, nodes, g_dev, self_loop=self_loop))
        assert bool((wide.grad[N:] == 0).all()), "table rows past num_nodes must get a zero gradient"
    with torch.no_grad():
        out = autograd.csr_mean_rows(rp, cl, table, nodes, index=batch.pos)
    assert not out.requires_grad and bits_equal(out, ops.csr_mean(rp, cl, table.detach(), nodes=nodes, index=batch.pos))
    out = autograd.csr_mean_rows(rp, cl, table.detach(), nodes, index=batch.pos)
    assert not out.requires_grad
    with pytest.raises(native.SageError):                          # the whole-graph wrapper keeps its refusal
        autograd.csr_mean(rp, cl, wide, nodes=nodes)
