"""A registry of operator cases for the execution-context tests (tests/test_gpu_operator_contexts.py): one small case per public
per-step operator, to be run off the default stream, with host synchronisation forbidden, under graph capture and on a second GPU.

A case builds a State on one device: the operator's inputs at ONE small shape, three sets of contents for them (0: the real ones,
1: a decoy, 2: a third set, with another n_dev where the operator takes one) that are written IN PLACE by device-to-device copies
(State.fill: nothing is allocated, nothing read back), every output and workspace preallocated wherever the wrapper takes out= /
workspace= / max_edges=, and call(), which enqueues the operator on torch's current stream and returns its output tensors.
The shapes are the smallest that still take the operator's multi-launch path: 65 rows (two 32-row tiles and a bit, two waves), a
CSR row and a transposed row past the 512-entry chunk (plan, chunk and row kernels run), k = 9 sets (the sorts run).

CLAIMS / EXCLUDED together must cover native.SYMBOLS: tests/test_operator_contexts_host.py fails for an entry point in neither.
Nothing here needs a GPU to be imported; build(device) does."""
import collections

import numpy as np
import torch

from sage355 import native, ops

SENTINEL_F, SENTINEL_I, STALE_BYTE = -777.25, -7, 0xA5
N, E, DIM, K = 65, 1100, 36, 9
LONG, HOT = (7, 40, 64), (3, 50, 21)             # per variant: the row that holds the graph's long list; the id most entries name
N_DEV = (63, 41, 65)
GROUPS = 7                                       # rows of the shared embedding of the indexed forms
SETS_ROWS = 200                                  # table rows the sampled sets name
WIDE, H = 256, 128                               # the contraction cases: dim 256, concat, 128 outputs (LDS above 64 KB)
HEAD_C = 64                                      # xent_head at 64 classes x 256 columns: its large-LDS form (147 KB)
VARIANTS = (0, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ contents (numpy)
def graph_variant(v):
    """(rowptr int64 [N + 1], col int32 [E]): every row but LONG[v] has 0..8 entries, LONG[v] the rest of the E (at least 588: two
    chunks or more); 60 % of the entries name HOT[v], so that row of the transpose (and its group) is past a chunk too."""
    rs = np.random.default_rng(500 + v)
    deg = rs.integers(0, 9, N)
    deg[LONG[v]] = 0
    deg[LONG[v]] = E - deg.sum()
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = np.where(rs.random(E) < 0.6, HOT[v], rs.integers(0, N, E)).astype(np.int32)
    return rowptr, col


def sets_variant(v, rows=SETS_ROWS, n=N, k=K):
    """Sampled sets over `rows` table rows: (nbr int32 [n, k], cnt int32 [n] with k, 0 and 1 among them, self_row int32 [n], -1 = none)"""
    rs = np.random.default_rng(700 + v)
    nbr = rs.integers(0, rows, (n, k)).astype(np.int32)
    cnt = rs.integers(0, k + 1, n).astype(np.int32)
    cnt[:3] = (k, 0, 1)
    self_row = rs.integers(0, rows, n).astype(np.int32)
    self_row[::5] = -1
    return nbr, cnt, self_row


def _f32(v, salt, *shape):
    return np.random.default_rng(1000 * salt + v).standard_normal(shape).astype(np.float32)


def _nodes(v, count=50, must=None):
    """`count` distinct node ids in random order, `must` (default LONG[v], the long row) among them (distinct: max_edges = E bounds
    their entries)"""
    must = LONG[v] if must is None else must
    perm = np.random.default_rng(900 + v).permutation(N)
    perm = perm[perm != must]
    return np.concatenate([perm[:5], [must], perm[5:count - 1]]).astype(np.int32)


def _index(v):
    idx = np.random.default_rng(1100 + v).integers(0, GROUPS, N).astype(np.int32)
    idx[HOT[v]] = v                                       # the hot node's group differs by variant
    return idx


def _n_dev(v):
    return np.asarray([N_DEV[v]], dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------ the state of a case
def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


class State:
    """One case on one device (see the module's docstring)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.inputs, self.contents = {}, [{}, {}, {}]
        self.outs, self.scratch = [], []
        self.call = None
        self.canon = lambda outs: list(outs)              # outputs (CPU copies, after a synchronise) -> what is compared bit for bit
        self.judge = None                                 # (variant, canon of outputs) -> None or a message: replaces the bit comparison

    def add(self, name, per_variant):
        """An input by name with its three contents (numpy arrays or CPU tensors of one shape and dtype) -> the device tensor."""
        ts = [(torch.from_numpy(np.ascontiguousarray(c)) if isinstance(c, np.ndarray) else c).to(self.device) for c in per_variant]
        assert len(ts) == 3 and all(t.shape == ts[0].shape and t.dtype == ts[0].dtype for t in ts), name
        self.inputs[name] = torch.empty_like(ts[0])
        for v in VARIANTS:
            self.contents[v][name] = ts[v]
        return self.inputs[name]

    def out(self, *shape, dtype=torch.float32):
        t = torch.empty(shape, dtype=dtype, device=self.device)
        self.outs.append(t)
        return t

    def workspace(self, nbytes):
        assert nbytes > 0, "the shape is out of the operator's range"
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.scratch.append(t)
        return t

    def fill(self, v):
        """Contents `v` into the inputs, in place, on the current stream."""
        for name, t in self.inputs.items():
            t.copy_(self.contents[v][name], non_blocking=True)

    def poison(self):
        """Sentinels into the preallocated outputs, stale bytes into the workspaces, on the current stream."""
        for t in self.outs:
            t.fill_(SENTINEL_F if t.is_floating_point() else SENTINEL_I)
        for t in self.scratch:
            t.fill_(STALE_BYTE)

    def verdict(self, v, got, want):
        """None when outputs `got` are what contents `v` must give -- the bits of `want` (outputs of a trusted call), or the case's own
        bound -- else a message.  got, want: lists of CPU tensors as call() returned them."""
        got = self.canon(got)
        if self.judge is not None:
            return self.judge(v, got)
        want = self.canon(want)
        bad = [i for i, (a, b) in enumerate(zip(got, want)) if not same_bits(a, b)]
        return None if not bad and len(got) == len(want) else f"outputs {bad} differ from the expected bits"


Case = collections.namedtuple("Case", "name claims build")
CASES = []


def case(name, *claims):
    def register(build):
        CASES.append(Case(name, tuple("sage_" + c for c in claims), build))
        return build
    return register


def _graph_inputs(st, transposed=False, grouped=False):
    gs = [graph_variant(v) for v in VARIANTS]
    rowptr, col = st.add("rowptr", [g[0] for g in gs]), st.add("col", [g[1] for g in gs])
    if transposed:
        ts = [ops.csr_transpose(torch.from_numpy(g[0]), torch.from_numpy(g[1])) for g in gs]
        assert all(int((t[0][1:] - t[0][:-1]).max()) > native.CSR_MEAN_CHUNK for t in ts)
        return rowptr, col, st.add("rowptr_t", [t[0] for t in ts]), st.add("col_t", [t[1] for t in ts])
    if grouped:
        ts = [ops.csr_transpose_grouped(torch.from_numpy(g[0]), torch.from_numpy(g[1]), torch.from_numpy(_index(v)), GROUPS) for v, g in enumerate(gs)]
        assert all(int((t.rowptr[1:] - t.rowptr[:-1]).max()) > native.CSR_MEAN_CHUNK for t in ts)
        return rowptr, col, ops.GroupedTranspose(st.add("rowptr_gt", [t.rowptr for t in ts]), st.add("col_gt", [t.col for t in ts]), False)
    return rowptr, col


# ------------------------------------------------------------------------------------------------------------------ the CSR family
def _csr_mean(st, table, **kw):
    rowptr, col = _graph_inputs(st)
    flag = st.add("any_nonempty", [np.zeros(1, np.int32)] * 3)
    nodes = st.add("nodes", [_nodes(v) for v in VARIANTS]) if kw.pop("with_nodes", False) else None
    n = N if nodes is None else nodes.shape[0]
    out = st.out(n, DIM)
    ws = st.workspace(ops.csr_mean_workspace_bytes(n, E, DIM))
    st.call = lambda: (ops.csr_mean(rowptr, col, table, nodes=nodes, self_loop=True, any_nonempty=flag, out=out, max_edges=E, workspace=ws, **kw),
                       flag)
    return st


@case("csr_mean", "csr_mean", "csr_mean_workspace_bytes")
def _(dev):
    st = State(dev)
    return _csr_mean(st, st.add("table", [_f32(v, 1, N, DIM) for v in VARIANTS]))


@case("csr_mean[bf16]", "csr_mean_bf16")
def _(dev):
    st = State(dev)
    return _csr_mean(st, st.add("table", [torch.from_numpy(_f32(v, 1, N, DIM)).to(torch.bfloat16) for v in VARIANTS]))


@case("csr_mean[index]", "csr_mean_indexed")
def _(dev):
    st = State(dev)
    return _csr_mean(st, st.add("embed", [_f32(v, 2, GROUPS, DIM) for v in VARIANTS]), index=st.add("index", [_index(v) for v in VARIANTS]))


@case("csr_mean[nodes]", "csr_mean")
def _(dev):
    st = State(dev)
    return _csr_mean(st, st.add("table", [_f32(v, 1, N, DIM) for v in VARIANTS]), with_nodes=True)


@case("csr_mean_backward", "csr_mean_backward", "csr_mean_backward_workspace_bytes")
def _(dev):
    st = State(dev)
    rowptr, col, rowptr_t, col_t = _graph_inputs(st, transposed=True)
    grad = st.add("grad_out", [_f32(v, 3, N, DIM) for v in VARIANTS])
    nodes = st.add("nodes", [_nodes(v, must=HOT[v]) for v in VARIANTS])      # the long row of the transpose is among the selected rows
    out = st.out(nodes.shape[0], DIM)
    ws = st.workspace(ops.csr_mean_backward_workspace_bytes(N, nodes.shape[0], E, DIM))
    st.call = lambda: (ops.csr_mean_backward(rowptr, col, rowptr_t, col_t, grad, nodes=nodes, self_loop=True, out=out, max_edges=E, workspace=ws),)
    return st


@case("csr_mean_backward_grouped", "csr_mean_backward_grouped", "csr_mean_backward_grouped_workspace_bytes")
def _(dev):
    st = State(dev)
    rowptr, col, grouped = _graph_inputs(st, grouped=True)
    grad = st.add("grad_out", [_f32(v, 3, N, DIM) for v in VARIANTS])
    out = st.out(GROUPS, DIM)
    ws = st.workspace(ops.csr_mean_backward_grouped_workspace_bytes(N, GROUPS, E, DIM))
    st.call = lambda: (ops.csr_mean_backward_grouped(rowptr, col, grouped, grad, out=out, max_edges=E, workspace=ws),)
    return st


def _seed_batch(st):
    rowptr, col = _graph_inputs(st)
    nodes = st.add("nodes", [_nodes(v) for v in VARIANTS])
    n = nodes.shape[0]
    grad = st.add("grad_out", [_f32(v, 4, n, DIM) for v in VARIANTS])
    return dict(rowptr=rowptr, col=col, nodes=nodes, grad_out=grad, self_loop=True, max_edges=E, total_terms=st.out(1, dtype=torch.int64)), n


@case("csr_mean_backward_rows", "csr_mean_backward_rows", "csr_mean_backward_rows_workspace_bytes")
def _(dev):
    st = State(dev)
    kw, n = _seed_batch(st)
    out = st.out(N, DIM)
    ws = st.workspace(ops.csr_mean_backward_rows_workspace_bytes(n, E, N, DIM))
    st.call = lambda: (ops.csr_mean_backward_rows(out=out, workspace=ws, **kw), kw["total_terms"])
    return st


@case("csr_mean_backward_touched", "csr_mean_backward_touched", "csr_mean_backward_touched_workspace_bytes")
def _(dev):
    st = State(dev)
    kw, n = _seed_batch(st)
    out = (st.out(N, dtype=torch.int32), st.out(1, dtype=torch.int32), st.out(N, DIM))
    ws = st.workspace(ops.csr_mean_backward_touched_workspace_bytes(n, E, N, DIM))
    st.call = lambda: ops.csr_mean_backward_touched(max_rows=N, out=out, workspace=ws, **kw) + (kw["total_terms"],)
    return st


@case("csr_sum", "csr_sum", "csr_sum_workspace_bytes")
def _(dev):
    st = State(dev)
    rowptr, col = _graph_inputs(st)
    table = st.add("table", [_f32(v, 1, N, DIM) for v in VARIANTS])
    out = st.out(N, DIM)
    ws = st.workspace(ops.csr_sum_workspace_bytes(N, E, DIM))
    st.call = lambda: (ops.csr_sum(rowptr, col, table, out=out, max_edges=E, workspace=ws),)
    return st


@case("pagerank_step", "pagerank_load", "pagerank_step", "pagerank_workspace_bytes")
def _(dev):
    st = State(dev)
    rowptr, col = _graph_inputs(st)
    xs, invs = [], []
    for v in VARIANTS:
        rs = np.random.default_rng(1300 + v)
        x = rs.random(N).astype(np.float32)
        xs.append(x / x.sum())
        inv = (1.0 / rs.integers(1, 9, N)).astype(np.float32)
        inv[rs.random(N) < 0.2] = 0.0                     # dangling nodes
        invs.append(inv)
    x, inv_out = st.add("x", xs), st.add("inv_out", invs)
    ws = st.workspace(ops.pagerank_workspace_bytes(N, E))
    st.call = lambda: ops.pagerank_step(rowptr, col, x, inv_out, alpha=0.85, workspace=ws)
    return st


@case("csr_cheb_step", "csr_cheb_step")
def _(dev):
    """On a plan made once (variant 0's graph, at build time): the contents that change are y and x."""
    st = State(dev)
    rowptr, col = (torch.from_numpy(a).to(st.device) for a in graph_variant(0))
    plan = ops.csr_cheb_plan(rowptr, col, DIM)
    torch.cuda.synchronize(st.device)
    y, x = st.add("y", [_f32(v, 5, N, DIM) for v in VARIANTS]), st.add("x", [_f32(v, 6, N, DIM) for v in VARIANTS])
    out = st.out(N, DIM)
    st.call = lambda: (ops.csr_cheb_step(plan, y, x=x, a=0.5, b=-0.25, g=0.125, out=out),)
    return st


def _set_canon(count, nodes, first_row=0):
    c = int(count[0])
    return [count, torch.sort(nodes[first_row:c].to(torch.int64)).values]


@case("csr_frontier", "csr_frontier", "csr_frontier_clear", "csr_frontier_workspace_bytes")
def _(dev):
    """clear + csr_frontier.  The set's order is the device's choice: compared are the count, the sorted ids and that pos maps each
    id to the row that holds it.  The frontier's state lives across calls, so none of it is poisoned."""
    st = State(dev)
    rowptr, col = _graph_inputs(st)
    seeds = st.add("seeds", [np.concatenate([_nodes(v)[:19], _nodes(v)[:1]]) for v in VARIANTS])      # the long row, one repeat
    fr = ops.CsrFrontier(N, st.device)
    fr.workspace = st.workspace(ops.csr_frontier_workspace_bytes(seeds.shape[0], E))

    def call():
        fr.clear()
        ops.csr_frontier(rowptr, col, seeds, fr, max_edges=E)
        return fr.count, fr.nodes, fr.pos

    def canon(outs):
        count, nodes, pos = outs
        ids = torch.nonzero(pos >= 0).flatten()
        return _set_canon(count, nodes) + [ids, nodes[pos[ids].long()].to(torch.int64)]
    st.call, st.canon = call, canon
    return st


# ------------------------------------------------------------------------------------------------------------------ samplers, frontier
def _sampler(dev, fn, k, with_frontier):
    st = State(dev)
    rowptr, col = _graph_inputs(st)
    nodes = st.add("nodes", [np.random.default_rng(1400 + v).permutation(N).astype(np.int32) for v in VARIANTS])
    n_dev = st.add("n_dev", [_n_dev(v) for v in VARIANTS])
    flag = st.add("any_nonempty", [np.zeros(1, np.int32)] * 3)
    out_nbr, out_cnt = st.out(N, k, dtype=torch.int32), st.out(N, dtype=torch.int32)
    kw = dict(k=k, seed=0x5EED1234, tag=ops.TAG_OUTER, n_dev=n_dev, any_nonempty=flag, out_nbr=out_nbr, out_cnt=out_cnt)
    if not with_frontier:
        st.call = lambda: fn(rowptr, col, nodes, **kw)[:2] + (flag,)
        return st
    fr = ops.Frontier(N * (k + 1), st.device)

    def call():
        fr.reset(0)
        nbr, cnt, slot, self_slot = fn(rowptr, col, nodes, frontier=fr, insert_self=True, **kw)
        return nbr, cnt, flag, slot, self_slot, fr.count, fr.nodes, fr.rows, n_dev, nodes
    st.call, st.canon = call, _frontier_canon
    return st


def _frontier_canon(outs):
    """The lists and the flag as they are; of the frontier (whose rows are handed out in the device's order) the count, the sorted
    ids, and the ids that the slots of the live rows' entries and self nodes lead to -- the entries and the nodes themselves."""
    nbr, cnt, flag, slot, self_slot, count, listed, rows, n_dev, nodes = outs
    live = min(int(n_dev[0]), nbr.shape[0])
    valid = (torch.arange(nbr.shape[1])[None, :] < cnt[:live, None])
    via = listed[rows[slot[:live][valid].long()].long()]
    res = [nbr, cnt] + ([] if flag is None else [flag]) + _set_canon(count, listed) + [via, nbr[:live][valid]]
    if self_slot is not None:
        res += [listed[rows[self_slot[:live].long()].long()], nodes[:live]]
    return res


@case("sample_neighbors", "sample_neighbors")
def _(dev):
    return _sampler(dev, ops.sample_neighbors, K, False)


@case("sample_neighbors[frontier]", "sample_neighbors", "frontier_reset")
def _(dev):
    return _sampler(dev, ops.sample_neighbors, K, True)


@case("sample_neighbors_wide", "sample_neighbors_wide")
def _(dev):
    return _sampler(dev, ops.sample_neighbors_wide, 70, False)


@case("sample_neighbors_wide[frontier]", "sample_neighbors_wide", "frontier_reset")
def _(dev):
    return _sampler(dev, ops.sample_neighbors_wide, 70, True)


@case("frontier_insert", "frontier_insert", "frontier_reset")
def _(dev):
    st = State(dev)
    sets = [sets_variant(v, rows=1000) for v in VARIANTS]
    nbr, cnt = st.add("nbr", [s[0] for s in sets]), st.add("cnt", [s[1] for s in sets])
    nodes = st.add("self_nodes", [np.random.default_rng(1500 + v).integers(0, 1000, N).astype(np.int32) for v in VARIANTS])
    n_dev = st.add("n_dev", [_n_dev(v) for v in VARIANTS])
    fr = ops.Frontier(N * (K + 1), st.device)

    def call():
        fr.reset(0)
        slot, self_slot = ops.frontier_insert(nbr, cnt, fr, self_nodes=nodes, n_dev=n_dev)
        return nbr, cnt, None, slot, self_slot, fr.count, fr.nodes, fr.rows, n_dev, nodes
    st.call, st.canon = call, _frontier_canon
    return st


# ------------------------------------------------------------------------------------------------------------------ sampled-set operators
def _set_inputs(st, rows=SETS_ROWS, self_rows=True):
    sets = [sets_variant(v, rows=rows) for v in VARIANTS]
    return (st.add("nbr", [s[0] for s in sets]), st.add("cnt", [s[1] for s in sets]),
            st.add("self_row", [s[2] for s in sets]) if self_rows else None, st.add("n_dev", [_n_dev(v) for v in VARIANTS]))


@case("gather_mean", "gather_mean")
def _(dev):
    st = State(dev)
    table = st.add("table", [_f32(v, 7, SETS_ROWS, 64) for v in VARIANTS])
    nbr, cnt, self_row, n_dev = _set_inputs(st)
    flag = st.add("any_nonempty", [np.zeros(1, np.int32)] * 3)
    out = st.out(N, 64)
    st.call = lambda: (ops.gather_mean(table, nbr, cnt, self_row=self_row, any_nonempty=flag, n_dev=n_dev, out=out), flag)
    return st


def _mean_backward_reference(v, grad):
    """fp64 (sum, sum of magnitudes) [SETS_ROWS, dim] of the terms grad[r] / c_r that the live rows' sets scatter (the self row joins a
    set that does not hold it) -- tests/test_gpu_backward_kernels.py's Mean.matrix on in-range ids."""
    nbr, cnt, self_row = sets_variant(v)
    want, mass = np.zeros((SETS_ROWS, grad.shape[1])), np.zeros((SETS_ROWS, grad.shape[1]))
    for r in range(min(N_DEV[v], N)):
        ids = [int(x) for x in nbr[r, :cnt[r]]]
        if self_row[r] >= 0 and int(self_row[r]) not in ids:
            ids.append(int(self_row[r]))
        for t in ids:
            want[t] += grad[r].astype(np.float64) / len(ids)
            mass[t] += np.abs(grad[r].astype(np.float64)) / len(ids)
    return want, mass


@case("gather_mean_backward", "gather_mean_backward")
def _(dev):
    """fp32 atomics: the order of additions is not fixed, so every context is judged against fp64 with the bound of
    tests/test_gpu_backward_kernels.py (|err| <= 1e-5 x the sum of the terms' magnitudes; an element without a term is exactly 0).
    The operator accumulates: the call zeroes its output first, on the same stream."""
    st = State(dev)
    grads = [_f32(v, 8, N, 64) for v in VARIANTS]
    grad = st.add("grad_out", grads)
    nbr, cnt, self_row, n_dev = _set_inputs(st)
    out = st.out(SETS_ROWS, 64)
    refs = [_mean_backward_reference(v, grads[v]) for v in VARIANTS]

    def call():
        out.zero_()
        return (ops.gather_mean_backward(grad, nbr, cnt, SETS_ROWS, self_row=self_row, n_dev=n_dev, out=out),)

    def judge(v, got):
        want, mass = refs[v]
        err = np.abs(got[0].double().numpy() - want)
        if np.any(got[0].numpy()[mass == 0] != 0):
            return "an element without a term is not 0"
        worst = float((err / np.maximum(mass, 1e-300))[mass > 0].max())
        return None if worst <= 1e-5 else f"max |err| / sum|terms| = {worst:.3e} > 1e-5"
    st.call, st.judge = call, judge
    return st


@case("gather_mean_backward_ws", "gather_mean_backward_ws", "gather_mean_backward_workspace_bytes")
def _(dev):
    """The reproducible adjoint (sorted terms, no atomics), through the C entry as the engine calls it: stored, bit for bit."""
    st = State(dev)
    grad = st.add("grad_out", [_f32(v, 8, N, 64) for v in VARIANTS])
    nbr, cnt, self_row, n_dev = _set_inputs(st)
    out = st.out(SETS_ROWS, 64)
    L, P = native.lib(), native.ptr
    ws = st.workspace(L.sage_gather_mean_backward_workspace_bytes(N, K, SETS_ROWS))

    def call():
        native.check(L.sage_gather_mean_backward_ws(P(grad), grad.stride(0), 64, P(nbr), P(cnt), K, N, P(n_dev), None, P(self_row), P(out),
                                                    SETS_ROWS, None, out.stride(0), P(ws), ws.numel(), native.stream_handle()),
                     "gather_mean_backward_ws")
        return (out,)
    st.call = call
    return st


@case("row_order", "row_order", "row_order_workspace_bytes")
def _(dev):
    st = State(dev)
    nodes = st.add("nodes", [np.random.default_rng(1600 + v).integers(0, 40, N).astype(np.int32) for v in VARIANTS])      # ids repeat
    n_dev = st.add("n_dev", [_n_dev(v) for v in VARIANTS])
    out = st.out(N, dtype=torch.int32)
    ws = st.workspace(ops.row_order_workspace_bytes(N))
    st.call = lambda: (ops.row_order(nodes, n_dev=n_dev, first_row=3, out=out, workspace=ws),)
    return st


def _embed_inputs(st, rows=50):
    grad = st.add("grad_agg", [_f32(v, 9, N, DIM) for v in VARIANTS])
    nbr, cnt, _, n_dev = _set_inputs(st, rows=rows, self_rows=False)
    order = st.add("row_order", [np.random.default_rng(1700 + v).permutation(N).astype(np.int32) for v in VARIANTS])
    return dict(grad_agg=grad, nbr=nbr, cnt=cnt, embed_rows=rows, n_dev=n_dev, row_order=order)


@case("embed_grad", "embed_grad", "embed_grad_workspace_bytes")
def _(dev):
    st = State(dev)
    kw = _embed_inputs(st)
    out = st.out(50, DIM)
    ws = st.workspace(ops.embed_grad_workspace_bytes(N, K, 50, DIM))
    st.call = lambda: (ops.embed_grad(out=out, workspace=ws, **kw),)
    return st


@case("embed_grad_rows", "embed_grad_rows", "embed_grad_rows_workspace_bytes")
def _(dev):
    st = State(dev)
    kw = _embed_inputs(st)
    out = (st.out(50, dtype=torch.int32), st.out(1, dtype=torch.int32), st.out(50, DIM))
    ws = st.workspace(ops.embed_grad_rows_workspace_bytes(N, K, 50, DIM))
    st.call = lambda: ops.embed_grad_rows(max_rows=50, out=out, workspace=ws, **kw)
    return st


# ------------------------------------------------------------------------------------------------------------------ contractions, head
def _linear_inputs(st):
    agg = st.add("agg", [_f32(v, 10, N, WIDE) for v in VARIANTS])
    self_tab = st.add("self_tab", [_f32(v, 11, N, WIDE) for v in VARIANTS])
    weight = st.add("weight", [_f32(v, 12, H, 2 * WIDE) / 16 for v in VARIANTS])
    return agg, weight, self_tab, st.add("n_dev", [_n_dev(v) for v in VARIANTS])


@case("linear_act", "linear_act")
def _(dev):
    st = State(dev)
    agg, weight, self_tab, n_dev = _linear_inputs(st)
    out = st.out(N, H)
    st.call = lambda: (ops.linear_act(agg, weight, act=ops.ACT_RELU, self_tab=self_tab, n_dev=n_dev, out=out),)
    return st


@case("linear_act_backward", "linear_act_backward_ws", "linear_act_backward_workspace_bytes")
def _(dev):
    """The wrapper allocates grad_x itself (torch.empty) and the kernel stores its first n_dev rows: the rows past them are whatever
    the allocator handed out, so only the live rows are compared."""
    st = State(dev)
    agg, weight, self_tab, n_dev = _linear_inputs(st)
    fwd =[np.maximum(np.concatenate([_f32(v, 11, N, WIDE), _f32(v, 10, N, WIDE)], 1) @ (_f32(v, 12, H, 2 * WIDE) / 16).T, 0).astype(np.float32)
           for v in VARIANTS]
    out, grad = st.add("out", fwd), st.add("grad_out", [_f32(v, 13, N, H) for v in VARIANTS])
    ws = st.workspace(max(256, ops.linear_act_backward_workspace_bytes(N, WIDE, True, H)))
    st.call = lambda: ops.linear_act_backward(agg, weight, ops.ACT_RELU, out, grad, self_tab=self_tab, n_dev=n_dev, workspace=ws) + (n_dev,)
    st.canon = lambda outs: [outs[0], outs[1][:min(int(outs[2][0]), N)]]
    return st


@case("layer_forward", "layer_forward", "layer_forward_supported")
def _(dev):
    st = State(dev)
    assert ops.layer_forward_supported(WIDE, H, True)
    table = st.add("table", [_f32(v, 14, SETS_ROWS, WIDE) for v in VARIANTS])
    weight = st.add("weight", [_f32(v, 12, H, 2 * WIDE) / 16 for v in VARIANTS])
    nbr, cnt, self_row, n_dev = _set_inputs(st)
    self_index = st.add("self_index", [np.random.default_rng(1800 + v).integers(0, SETS_ROWS, N).astype(np.int32) for v in VARIANTS])
    flag = st.add("any_nonempty", [np.zeros(1, np.int32)] * 3)
    out = st.out(N, H)
    st.call = lambda: (ops.layer_forward(table, nbr, cnt, weight, act=ops.ACT_RELU, concat=True, self_index=self_index, self_row=self_row,
                                         any_nonempty=flag, n_dev=n_dev, out=out), flag)
    return st


@case("layer1_fused", "layer1_fused", "layer1_fused_supported", "prepare_weights", "prepared_weight_bytes")
def _(dev):
    """prepared=None: the weight's planes are prepared inside the call (sage_prepare_weights on the same stream), as a trainer does."""
    st = State(dev)
    assert ops.layer1_fused_supported(WIDE, H, K)
    sliced = st.add("table_sliced", [ops.slice_major(torch.from_numpy(_f32(v, 14, SETS_ROWS, WIDE))) for v in VARIANTS])
    weight = st.add("weight", [_f32(v, 15, H, WIDE) / 16 for v in VARIANTS])
    nbr, cnt, self_row, n_dev = _set_inputs(st)
    flag = st.add("any_nonempty", [np.zeros(1, np.int32)] * 3)
    out = st.out(N, H)
    st.call = lambda: (ops.layer1_fused(sliced, nbr, cnt, weight, act=ops.ACT_RELU, self_row=self_row, any_nonempty=flag, n_dev=n_dev, out=out), flag)
    return st


@case("xent_head", "xent_head", "xent_head_supported", "xent_head_workspace_bytes")
def _(dev):
    st = State(dev)
    emb = st.add("emb", [_f32(v, 16, N, WIDE) for v in VARIANTS])
    w_cls = st.add("w_cls", [_f32(v, 17, HEAD_C, WIDE) / 16 for v in VARIANTS])
    labels = st.add("labels", [np.random.default_rng(1900 + v).integers(0, HEAD_C, N) for v in VARIANTS])
    out = {"scores": st.out(N, HEAD_C), "pred": st.out(N, dtype=torch.int32), "loss": st.out(1), "grad_emb": st.out(N, WIDE),
           "grad_w": st.out(HEAD_C, WIDE)}
    ws = st.workspace(ops.xent_head_workspace_bytes(N, WIDE, HEAD_C))
    st.call = lambda: tuple(ops.xent_head(emb, w_cls, labels, scores=True, pred=True, grads=True, workspace=ws, out=out).values())
    return st


NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ------------------------------------------------------------------------------------------------------------------ what no case claims
_HOST_DRIVEN = "host-driven: its wrapper reads the device between launches by design (tests of its own compare it with the oracle)"
_BUILD_ONCE = "build-once: runs once per graph or model, never inside a step, a capture or a stream of steps"
_ENGINE = "a TwoHopEngine entry: the engine's own tests run it on side streams, under capture and on a second GPU"
_PIPE = "a RolePipeline entry: the pipeline owns its streams and threads, its own tests cover them"
_INFO = "host arithmetic or a constant: launches nothing"
EXCLUDED = {
    "sage_abi_version": _INFO, "sage_last_error": _INFO, "sage_build_arch": _INFO, "sage_forward2_layout": _INFO,
    "sage_two_hop_grad_w1_workspace_bytes": _INFO,
    "sage_pagerank_init": _HOST_DRIVEN + " (ops.pagerank: 4 bytes of err per iteration)",
    "sage_csr_cheb_plan": _BUILD_ONCE + " (ops.csr_cheb_plan; the csr_cheb_step case steps on a plan made at build time; ops.eigen_top, "
                          "which drives both, is host-driven)",
    "sage_csr_cheb_workspace_bytes": _INFO,
    "sage_forward2_init": _BUILD_ONCE + "; " + _ENGINE, "sage_forward2": _ENGINE, "sage_forward2_profiled": _ENGINE,
    "sage_two_hop_grad_w1": "EngineTrainer's layer-1 weight gradient over the engine's workspace layout: EngineTrainer.capture_step's tests "
                            "replay it under capture",
    "sage_linear_act_backward": "the atomic form of sage_linear_act_backward_ws: no wrapper of this package calls it",
    "sage_pipe_create": _PIPE, "sage_pipe_destroy": _PIPE, "sage_pipe_update_weights": _PIPE, "sage_pipe_submit": _PIPE,
    "sage_pipe_submit_profiled": _PIPE, "sage_pipe_submit_many": _PIPE, "sage_pipe_join": _PIPE, "sage_pipe_fork": _PIPE,
    "sage_pipe_reset": _PIPE, "sage_pipe_set_threads": _PIPE, "sage_pipe_flush": _PIPE, "sage_pipe_express_count": _PIPE,
    "sage_pipe_alternate_count": _PIPE, "sage_pipe_inner_with_layer1_count": _PIPE,
}
# wrappers of ops that are not per-step operators and own no entry point: named here so that the table is the whole answer
EXCLUDED_WRAPPERS = {
    "pagerank": _HOST_DRIVEN, "eigen_top": _HOST_DRIVEN, "csr_transpose": _BUILD_ONCE + " (torch operations with one host check of the ids)",
    "csr_transpose_grouped": _BUILD_ONCE + " (torch operations with one host check of the ids)",
    "group_rows": _BUILD_ONCE + " (torch operations with one host check of the index)",
    "embed_nodes": _HOST_DRIVEN + " (sage355.inference: layer-wise inference over batches, driven from the host)",
}


def claimed():
    """entry point -> the names of the cases that claim it"""
    res = collections.defaultdict(list)
    for c in CASES:
        for sym in c.claims:
            res[sym].append(c.name)
    return dict(res)
