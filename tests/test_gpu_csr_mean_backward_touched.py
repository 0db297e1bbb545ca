"""sage_csr_mean_backward_touched (sage_csr_mean_backward_rows for the touched table rows only, with the SGD update of those rows
fused in; include/sage355.h) on the MI355X.

The graph and the batch are tests/test_gpu_csr_mean_backward_rows.py's (the builder is copied): 6000 nodes, about 2095 shuffled seed
rows -- more than one 2048-row count tile -- with targets that receive 0, 1, 63, 64, 65, 511, 512, 513, 1025 and 1537 terms, a
1537-entry seed row, a repeated seed, a duplicate neighbour, seeds inside their own rows, empty rows and one id outside the graph:
about 10^4 term positions, more than four 2048-position run-head tiles.  Five indices send the terms to table rows:
  frontier  the CsrFrontier map, R = |F|                     degree  index[v] = deg(v), R = max deg + 1 (runs of > 2 chunks, empty rows)
  one       R = 1: every term in one run of about 20 chunks   spread  frontier's rows increasingly into 37 |F| + 6 rows (0 and R - 1 hit)
  huge      the same into R = 2^31 - 2 rows: gradient only, in a workspace of exactly the queried size
1. U and rows_out are the ascending distinct keys of the host; 2. grad_rows is bit for bit csr_mean_backward_rows(...)[rows];
3. spread and huge give frontier's bits: they do not depend on where the rows lie; 4. dense rows outside rows_out are exact zeros;
5. against fp64 from the fp32 inputs and the fp32 weight: |got - want| <= gamma_m * sum|terms|, gamma_m = m u / (1 - m u), u = 2^-24,
   m = min(c, 512) + ceil(c / 512) + 1 for a row of c terms (the longest chain of additions is one chunk plus the chunk adds, and one
   rounding more for the weight: tests/test_gpu_embed_sparse.py's derived bound, a worst case the arithmetic cannot exceed);
6. the update: touched rows within one fp32 rounding of old - lr s, everything else (NaN canaries in the padding) keeps its bits;
7. a short max_rows still reports U and still updates all U rows; 8. a max_edges below the truth drops the parent's terms;
9. two calls give the same bits; 10. the wrapper's refusals."""
import numpy as np
import pytest
import torch

from sage355 import native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = native.CSR_MEAN_CHUNK
U32 = 2.0 ** -24
SENTINEL = -31.5
COUNTS = (0, 1, 63, 64, 65, 511, 512, 513, 1025, 1537)
N = 6000
HUGE = (1 << 31) - 2
KINDS = ("frontier", "degree", "one", "spread", "huge")
CASES = [(1, 0), (3, 0), (4, 0), (12, 3), (12, 4), (260, 0), (260, 4)]        # (dim, padding of every leading dimension)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def build_graph():
    """tests/test_gpu_csr_mean_backward_rows.py's builder: filler seed i names target t_c exactly when i < c."""
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
    return rowptr, col, batch, dict(targets=targets, hub=hub, lonely=lonely)


def host_terms(rowptr, col, nodes, self_loop):
    """The batch's terms in the documented order -> (node id of every term, seed row of every term, w [m] fp32)."""
    ids, vals = [], []
    w = np.zeros(len(nodes), dtype=np.float32)
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
    return np.concatenate(ids), np.concatenate(vals), w


class Batch:
    def __init__(self):
        self.rowptr, self.col, self.nodes, self.who = build_graph()
        self.m = len(self.nodes)
        self.dev = tuple(torch.from_numpy(x).to(DEV) for x in (self.rowptr, self.col, self.nodes))
        self.entries = int(sum(self.rowptr[v + 1] - self.rowptr[v] for v in self.nodes.tolist() if 0 <= v < N))
        fr = ops.CsrFrontier(N, DEV)
        ops.csr_frontier(self.dev[0], self.dev[1], self.dev[2], fr)
        f = fr.size()
        pos = fr.pos.cpu().numpy().astype(np.int64)
        deg = np.diff(self.rowptr)

        def stretched(rows, step):                                # frontier row j -> j * step, the last one -> rows - 1: increasing
            image = np.arange(f, dtype=np.int64) * step
            image[-1] = rows - 1
            assert (np.diff(image) > 0).all() and image[0] == 0
            return np.where(pos >= 0, image[np.maximum(pos, 0)], -1)

        self.index = {"frontier": (pos, f), "degree": (deg, int(deg.max()) + 1), "one": (np.zeros(N, dtype=np.int64), 1),
                      "spread": (stretched(37 * f + 6, 37), 37 * f + 6), "huge": (stretched(HUGE, (HUGE - 1) // (f - 1)), HUGE)}
        self.index_dev = {k: torch.from_numpy(v[0].astype(np.int32)).to(DEV) for k, v in self.index.items()}
        self.terms = {s: host_terms(self.rowptr, self.col, self.nodes, s) for s in (False, True)}

    def keys(self, kind, self_loop):
        index, rows = self.index[kind]
        return np.clip(index[self.terms[self_loop][0]], 0, rows - 1)

    def rows_of(self, kind):
        return self.index[kind][1]

    def touched(self, g_dev, kind, self_loop, **kw):
        rp, cl, nodes = self.dev
        return ops.csr_mean_backward_touched(rp, cl, nodes, g_dev, index=self.index_dev[kind], num_rows=self.rows_of(kind), self_loop=self_loop, **kw)

    def dense(self, g_dev, kind, self_loop, **kw):
        rp, cl, nodes = self.dev
        return ops.csr_mean_backward_rows(rp, cl, nodes, g_dev, index=self.index_dev[kind], num_rows=self.rows_of(kind), self_loop=self_loop, **kw)

    def reference(self, g, kind, self_loop):
        """(rows [U], want, A fp64 [U, dim], c [U] terms per row) from the fp32 inputs with the fp32 weight."""
        _, vals, w = self.terms[self_loop]
        rows, inv, c = np.unique(self.keys(kind, self_loop), return_inverse=True, return_counts=True)
        term = g.double().numpy()[vals] * w.astype(np.float64)[vals, None]
        want = np.zeros((len(rows), g.shape[1]))
        A = np.zeros_like(want)
        np.add.at(want, inv, term)
        np.add.at(A, inv, np.abs(term))
        return rows, want, A, c


@pytest.fixture(scope="module")
def batch():
    b = Batch()
    assert 2050 <= b.m <= 2150 and b.m > 2048, "more than one count tile of seed rows"
    for self_loop in (False, True):
        assert len(b.terms[self_loop][0]) > 4 * 2048, "more than four run-head tiles of term positions"
    per_row = np.bincount(b.keys("frontier", False), minlength=b.rows_of("frontier"))
    pos = b.index["frontier"][0]
    for c, t in b.who["targets"].items():
        assert per_row[pos[t]] == c, (c, per_row[pos[t]])
    assert per_row[pos[b.who["lonely"]]] == 0 and set(COUNTS) <= set(per_row.tolist())
    per_degree = np.bincount(b.keys("degree", False), minlength=b.rows_of("degree"))
    assert per_degree.max() > 2 * E and (per_degree == 0).any(), "degree: a run of more than two chunks and a row without a term"
    assert len(b.keys("one", True)) > 19 * E
    for kind in ("spread", "huge"):
        k = b.keys(kind, True)
        assert k.min() == 0 and k.max() == b.rows_of(kind) - 1, f"{kind}: images at row 0 and at row R - 1"
    return b


def _grad(n, dim, pad, seed):
    """grad_out [n, dim] on the CPU and its device copy with leading dimension dim + pad (the padding holds the sentinel)."""
    g = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))
    wide = torch.full((n, dim + pad), SENTINEL)
    wide[:, :dim] = g
    return g, (wide.to(DEV)[:, :dim] if pad else wide.to(DEV))


def _outputs(cap, dim, pad, guard=2):
    """(rows, num_rows, grad_rows) filled with sentinels: `guard` rows past cap, `pad` columns past dim."""
    rows = torch.full((cap + guard,), -7, dtype=torch.int32, device=DEV)
    grad = torch.full((cap + guard, dim + pad), SENTINEL, device=DEV)
    return rows, torch.full((1,), -7, dtype=torch.int32, device=DEV), grad


def _bound(A, c):
    m = np.minimum(c, 512) + np.ceil(c / 512) + 1
    return (m * U32 / (1 - m * U32))[:, None] * A


_frontier_bits = {}


@pytest.mark.parametrize("dim,pad", CASES)
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_the_touched_rows_and_their_gradient(batch, kind, self_loop, dim, pad):
    g, g_dev = _grad(batch.m, dim, pad, seed=dim + pad)
    want_rows, want, A, c = batch.reference(g, kind, self_loop)
    nu = len(want_rows)
    cap = min(batch.entries + batch.m, batch.rows_of(kind))
    out = _outputs(cap, dim, pad)
    total = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    kw = dict(max_edges=batch.entries, out=(out[0], out[1], out[2][:, :dim]), total_terms=total)
    if kind == "huge":                                            # a workspace of exactly the queried size
        need = ops.csr_mean_backward_touched_workspace_bytes(batch.m, batch.entries, HUGE, dim)
        assert need == ops.csr_mean_backward_touched_workspace_bytes(batch.m, batch.entries, batch.entries + batch.m, dim)
        kw["workspace"] = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
    rows, num, grad = batch.touched(g_dev, kind, self_loop, **kw)
    # 1. the rows
    assert int(num) == nu and int(total) == len(batch.terms[self_loop][0])
    assert np.array_equal(rows[:nu].cpu().numpy().astype(np.int64), want_rows), "rows_out is not the ascending distinct keys"
    assert bool((out[0][nu:] == -7).all()) and bool((out[2][nu:] == SENTINEL).all()) and bool((out[2][:, dim:] == SENTINEL).all()), \
        "something past row U or in the padding columns was written"
    got = grad[:nu]
    # 9. two calls
    again = batch.touched(g_dev, kind, self_loop, max_edges=batch.entries)
    assert int(again[1]) == nu and bits_equal(again[2][:nu], got) and torch.equal(again[0][:nu], rows[:nu]), "two calls differ"
    # 2. and 4. the dense entry's rows, and zeros everywhere else
    if kind != "huge":
        dense = batch.dense(g_dev, kind, self_loop, max_edges=batch.entries)
        assert bits_equal(got, dense[rows[:nu].long()]), "grad_rows differs from csr_mean_backward_rows' rows"
        rest = torch.ones(batch.rows_of(kind), dtype=torch.bool, device=DEV)
        rest[rows[:nu].long()] = False
        assert bool((dense[rest].view(torch.int32) == 0).all()), "a dense row outside rows_out is not exact zeros"
    # 3. the bits do not depend on where the rows lie
    if kind == "frontier":
        _frontier_bits[(self_loop, dim, pad)] = got.clone()
    if kind in ("spread", "huge"):
        ref = _frontier_bits.get((self_loop, dim, pad))
        if ref is None:
            ref = batch.touched(g_dev, "frontier", self_loop, max_edges=batch.entries)[2][:nu]
        assert bits_equal(got, ref), f"{kind}: the bits differ from the frontier map's"
    # 5. fp64
    if kind in ("frontier", "degree", "one"):
        err = np.abs(got.double().cpu().numpy() - want)
        bound = _bound(A, c)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{kind} self_loop={self_loop} dim={dim} pad={pad}: U = {nu}, longest run {int(c.max())}, max |got - want| = {err.max():.3e}, "
              f"max err / bound = {worst:.3f}")
        assert np.all(err <= bound), f"|got - want| exceeds gamma_m * sum|terms| (ratio {worst:.3f})"


def _table(rows, dim, pad, seed=7):
    table = torch.full((rows, dim + pad), float("nan"), device=DEV)                  # the canary in the padding columns
    table[:, :dim] = torch.randn(rows, dim, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return table


def fp64_update_check(new, old, g, lr, what):
    """|new - (old - lr g)| <= 2^-24 |old - lr g| (1 + 2^-20): one fp32 rounding of the exact value; the last factor covers the fp64
    reference's own rounding.  lr is the float32 the kernel is handed.  (tests/test_gpu_embed_sparse.py's check.)"""
    lr32 = float(np.float32(lr))
    ref = old.double() - lr32 * g.double()
    err = (new.double() - ref).abs()
    bound = U32 * ref.abs() * (1 + 2.0 ** -20)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |new - ref| = {float(err.max()):.3e}, max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: more than one rounding away from old - lr * g (ratio {worst:.3f})"


@pytest.mark.parametrize("lr", [0.7, 0.0])
@pytest.mark.parametrize("dim,pad", [(1, 0), (3, 2), (4, 4), (12, 0), (260, 4)])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("kind", ["frontier", "degree", "one", "spread"])
def test_the_update_touches_the_named_rows_once_and_nothing_else(batch, kind, self_loop, dim, pad, lr):
    _, g_dev = _grad(batch.m, dim, pad, seed=40 + dim)
    R = batch.rows_of(kind)
    table = _table(R, dim, pad)
    old = table.clone()
    rows, num, grad = batch.touched(g_dev, kind, self_loop, max_edges=batch.entries, table=table[:, :dim], lr=lr)
    nu = int(num)
    assert nu == len(np.unique(batch.keys(kind, self_loop)))
    only = batch.touched(g_dev, kind, self_loop, max_edges=batch.entries)
    assert bits_equal(grad[:nu], only[2][:nu]), "the gradient returned with an update is not the gradient-only call's"
    idx = rows[:nu].long()
    fp64_update_check(table[idx, :dim], old[idx, :dim], grad[:nu], lr, f"{kind} self_loop={self_loop} dim={dim} lr={lr}")
    rest = torch.ones(R, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert bits_equal(table[rest], old[rest]), "a row without a term changed"
    assert bool(torch.isnan(table[:, dim:]).all()), "a padding column was written"
    if lr == 0.0:
        assert bits_equal(table, old), "lr = 0 changed the table's bits"
    # the update-only form: the same table, no gradient
    table2 = old.clone()
    r2, n2, g2 = batch.touched(g_dev, kind, self_loop, max_edges=batch.entries, table=table2[:, :dim], lr=lr, want_grad=False)
    assert r2 is None and g2 is None and int(n2) == nu
    assert bits_equal(table2, table), "update-only and update + gradient give different tables"


@pytest.mark.parametrize("kind", ["frontier", "degree"])
def test_a_short_max_rows_still_reports_u_and_updates_every_row(batch, kind):
    dim, pad, self_loop, lr = 12, 4, True, 0.7
    _, g_dev = _grad(batch.m, dim, pad, seed=5)
    R = batch.rows_of(kind)
    full_table = _table(R, dim, pad)
    rows, num, grad = batch.touched(g_dev, kind, self_loop, max_edges=batch.entries, table=full_table[:, :dim], lr=lr)
    nu = int(num)
    assert nu > 2
    for max_rows in (1, nu - 1, nu):
        out = _outputs(max_rows, dim, pad)
        table = _table(R, dim, pad)
        r, n_, g_ = batch.touched(g_dev, kind, self_loop, max_edges=batch.entries, max_rows=max_rows, table=table[:, :dim], lr=lr,
                                  out=(out[0], out[1], out[2][:, :dim]))
        assert int(n_) == nu, "U must be reported whatever max_rows is"
        assert torch.equal(r[:max_rows], rows[:max_rows]) and bits_equal(g_[:max_rows], grad[:max_rows])
        assert bool((out[0][max_rows:] == -7).all()) and bool((out[2][max_rows:] == SENTINEL).all()), f"max_rows = {max_rows}: row max_rows written"
        assert bool((out[2][:, dim:] == SENTINEL).all())
        assert bits_equal(table, full_table), f"max_rows = {max_rows}: the update did not reach all U rows"


@pytest.mark.parametrize("self_loop", [False, True])
def test_a_max_edges_below_the_truth_drops_the_terms_the_parent_drops(batch, self_loop):
    dim = 12
    _, g_dev = _grad(batch.m, dim, 0, seed=9)
    for kind in ("frontier", "degree"):
        for short in (batch.entries - 1, batch.entries // 2):
            t_dense = torch.full((1,), -1, dtype=torch.int64, device=DEV)
            t_touched = t_dense.clone()
            dense = batch.dense(g_dev, kind, self_loop, max_edges=short, total_terms=t_dense)
            rows, num, grad = batch.touched(g_dev, kind, self_loop, max_edges=short, total_terms=t_touched)
            nu = int(num)
            assert int(t_touched) == int(t_dense) == len(batch.terms[self_loop][0]), "total_terms must report the true count"
            assert nu <= min(short + batch.m, batch.rows_of(kind))
            assert bits_equal(grad[:nu], dense[rows[:nu].long()]), "the dropped terms are not the parent's"
            rest = torch.ones(batch.rows_of(kind), dtype=torch.bool, device=DEV)
            rest[rows[:nu].long()] = False
            assert bool((dense[rest] == 0).all())
            assert bool((rows[1:nu] > rows[:nu - 1]).all())


def test_the_wrappers_conventions_and_refusals(batch):
    rp, cl, nodes = batch.dev
    dim = 8
    _, g_dev = _grad(batch.m, dim, 0, seed=11)
    index, R = batch.index_dev["frontier"], batch.rows_of("frontier")
    table = torch.zeros(R, dim, device=DEV)
    # no seed rows: the counts are zeroed in Python, nothing else is touched
    total = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    keep = table.clone().fill_(3.0)
    rows, num, grad = ops.csr_mean_backward_touched(rp, cl, torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dim, device=DEV),
                                                    index=index, num_rows=R, table=keep, lr=0.5, total_terms=total)
    assert int(num) == 0 and int(total) == 0 and bool((keep == 3.0).all())
    # index=None is the identity map over the nodes
    by_node = ops.csr_mean_backward_touched(rp, cl, nodes, g_dev)
    ident = ops.csr_mean_backward_touched(rp, cl, nodes, g_dev, index=torch.arange(N, dtype=torch.int32, device=DEV), num_rows=N)
    nu = int(by_node[1])
    assert nu == int(ident[1]) and torch.equal(by_node[0][:nu], ident[0][:nu]) and bits_equal(by_node[2][:nu], ident[2][:nu])
    assert by_node[0].shape[0] == min(batch.entries + batch.m, N), "default max_rows = min(max_edges + n, num_rows)"
    call = lambda **kw: ops.csr_mean_backward_touched(rp, cl, nodes, g_dev, **dict(dict(index=index, num_rows=R), **kw))
    for kw, word in [(dict(want_grad=False), "nothing to do"), (dict(table=table), "go together"), (dict(lr=0.1), "go together"),
                     (dict(num_rows=None), "num_rows is required"), (dict(index=index[:-1]), "entries"),
                     (dict(table=table[:, :4], lr=0.1), "table is"), (dict(table=table[:R - 1], lr=0.1), "table is"),
                     (dict(max_rows=0), "max_rows"), (dict(num_rows=0), "num_rows = 0"),
                     (dict(out=(torch.zeros(3, dtype=torch.int32, device=DEV), None, None)), "out is"),
                     (dict(total_terms=torch.zeros(1, dtype=torch.int32, device=DEV)), "total_terms")]:
        with pytest.raises(native.SageError, match=word):
            call(**kw)
    with pytest.raises(native.SageError):
        ops.csr_mean_backward_touched(rp, cl, nodes, g_dev[:5], index=index, num_rows=R)
    with pytest.raises(native.SageError):
        ops.csr_mean_backward_touched(rp, cl, nodes.long(), g_dev, index=index, num_rows=R)
