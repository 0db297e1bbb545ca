"""The pagerank initializer on the GPU: one step element-wise against fp64 at the kernel's edge shapes, whole runs against the
networkx goldens, bit reproducibility, the failure modes, and the [N, 1] table through the three trainers and the inference stack.

Bounds (u = 2^-24, D dangling nodes, len_i entries in row i), derived and not tuned:
    |x_next_i - ref_i| <= u * [(len_i + 8) * ref_i + alpha * D * mass / N]
        the row's sum of len_i non-negative terms in any order (len_i - 1 roundings), y = x * inv_out (1), + mass / N (1), the
        division behind it (1), the fma (1), (1 - alpha) / N (2), alpha as a float (1/2); the dangling mass is a sum of D terms
    |err - err_ref| <= 2 * sum_i bound_i + (N + 2) * u * err_ref
        a term moves by at most its x_next's bound and one rounding of the difference; N terms are added
    whole run: ||x - x_ref||_1 <= sum_i (len_i + 8) * u * x_ref_i / (1 - alpha)
        the step bound carried through the contraction (the map shrinks l1 distances by alpha); sum x = 1 to N * u."""
import os

import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.datasets import pagerank_table, standin_citation
from sage355.graph import CSRGraph
from test_pagerank_host import ALPHA, golden_cases, pagerank_fp64, step_fp64
from util import GOLDEN_DIR, assert_close_rowmax

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025, 3000]
TILE = 512                                                           # rows of one (err, mass) partial: csrc/sage_pagerank.hip kPrTile


def edge_graph(n, seed, edges=True):
    """N nodes whose rows have the EDGE_LENGTHS (as many of them as there are rows, from a seeded offset on) and 0..20 entries
    elsewhere; entries are random ids (a row may name a node twice: the kernel sums stored entries), rows 0, 3 and every 11th start
    with a self loop.  Random positive x (sum 1) and inv_out = 1 / k with about a fifth of the nodes dangling (inv_out = 0)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 21, n)
    where = rng.permutation(n)[:len(EDGE_LENGTHS)]
    lens[where] = np.roll(EDGE_LENGTHS, seed)[:len(where)]
    if not edges:
        lens[:] = 0
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    for r in range(n):
        if lens[r] > 0 and (r in (0, 3) or r % 11 == 0):
            col[rowptr[r]] = r
    x = rng.random(n).astype(np.float32) + np.float32(0.05)
    x /= x.sum(dtype=np.float64).astype(np.float32)
    inv_out = (1.0 / rng.integers(1, 40, n)).astype(np.float32)
    inv_out[rng.random(n) < 0.2] = 0.0
    return rowptr, col, x, inv_out


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


STEP_CASES = [(1, 1, True), (1, 0, False), (63, 2, True), (64, 3, True), (65, 4, True), (65, 5, False), (257, 6, True), (TILE + 1, 7, True),
              (2 * TILE + 3, 8, True)]


@pytest.mark.parametrize("n,seed,edges", STEP_CASES)
def test_one_step_against_fp64(n, seed, edges):
    rowptr, col, x, inv_out = edge_graph(n, seed, edges)
    lens = np.diff(rowptr)
    if edges and n >= 63:
        assert set(EDGE_LENGTHS) <= set(lens.tolist())
    ref, err_ref, mass = step_fp64(rowptr, col, x, inv_out, ALPHA)
    x_next, err = ops.pagerank_step(*dev(rowptr, col, x, inv_out), alpha=ALPHA)
    assert x_next.shape == (n,) and x_next.dtype == torch.float32 and err.shape == (1,) and err.is_cuda
    got = x_next.cpu().numpy().astype(np.float64)
    d = int((inv_out == 0).sum())
    bound = U * ((lens + 8) * ref + ALPHA * d * mass / n)
    ratio = np.abs(got - ref) / bound
    err_bound = 2 * bound.sum() + (n + 2) * U * err_ref
    print(f"N={n} entries={len(col)} dangling={d}: max |x_next - ref| / bound = {ratio.max():.3f}, |err - ref| / bound = "
          f"{abs(float(err) - err_ref) / err_bound:.3f}")
    assert np.all(ratio <= 1.0), (int(ratio.argmax()), float(ratio.max()))
    assert abs(float(err) - err_ref) <= err_bound


def test_a_row_has_the_bits_it_has_in_any_other_graph():
    """x_next[i] depends on row i's stored entries, y and the step's scalars alone: the rows of a graph keep their bits when the
    graph's row order is rotated (another block, another group, other neighbours in the wave), N, mass and y staying what they were."""
    n, shift = 2 * TILE + 3, 389
    rowptr, col, x, inv_out = edge_graph(n, 8)
    lens = np.diff(rowptr)
    a, _ = ops.pagerank_step(*dev(rowptr, col, x, inv_out))
    order = np.roll(np.arange(n), shift)                              # new row j is old row order[j]
    rowptr_r = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens[order], out=rowptr_r[1:])
    col_r = np.concatenate([col[rowptr[r]:rowptr[r + 1]] for r in order]).astype(np.int32)
    # y is gathered by id, so the ids keep their meaning: only the ROWS move.  x and inv_out stay indexed by id; row j's own
    # x and inv_out enter err and y_next only, never x_next
    b, _ = ops.pagerank_step(*dev(rowptr_r, col_r, x, inv_out))
    assert torch.equal(a[torch.from_numpy(order).cuda()].view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def cases():
    return golden_cases()


@pytest.fixture(scope="module")
def runs(cases):
    """Every golden case run once: (x, iterations, err history)."""
    out = {}
    for name, c in cases.items():
        hist = []
        x, it = ops.pagerank(*dev(c["rowptr"], c["col"]), symmetric=bool(c["symmetric"]), err_history=hist)
        out[name] = (x, it, hist)
    return out


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_whole_run_against_networkx(cases, runs, name):
    c = cases[name]
    x, it, hist = runs[name]
    n = len(c["rowptr"]) - 1
    assert x.shape == (n,) and x.dtype == torch.float32 and x.is_cuda
    assert it == int(c["iterations"]) and len(hist) == it
    got, ref = x.cpu().numpy().astype(np.float64), c["x"]
    lens = np.diff(c["rowptr"])
    if not bool(c["symmetric"]):                                     # the pull rows of out-edge lists are the in-edge lists
        lens = np.bincount(c["col"], minlength=n)
    l1, bound = np.abs(got - ref).sum(), ((lens + 8) * U * ref).sum() / (1 - ALPHA)
    print(f"case {name}: N={n} iterations={it} max relative error {float((np.abs(got - ref) / ref).max()):.2e}, l1 error / bound = "
          f"{l1 / bound:.3f}, |sum x - 1| = {abs(got.sum() - 1):.1e}, err {hist[-2]:.4e} -> {hist[-1]:.4e} (fp64 {c['err'][0]:.4e} -> {c['err'][1]:.4e})")
    assert l1 <= bound
    assert abs(got.sum() - 1.0) <= n * U


def test_two_calls_give_the_same_bits(cases, runs):
    for name in ("b", "d"):
        c = cases[name]
        hist = []
        x, it = ops.pagerank(*dev(c["rowptr"], c["col"]), symmetric=bool(c["symmetric"]), err_history=hist)
        assert it == runs[name][1] and hist == runs[name][2]
        assert torch.equal(x.view(torch.int32), runs[name][0].view(torch.int32))


def test_out_edge_lists_of_a_symmetric_graph_give_the_bits_of_its_own_rows(cases, runs):
    """symmetric=False pulls over csr_transpose, which for a symmetric graph is the graph's CSR again, entry for entry."""
    for name in ("a", "c"):
        c = cases[name]
        hist = []
        x, it = ops.pagerank(*dev(c["rowptr"], c["col"]), symmetric=False, err_history=hist)
        assert it == runs[name][1] and hist == runs[name][2]
        assert torch.equal(x.view(torch.int32), runs[name][0].view(torch.int32))


def test_no_convergence_raises_and_bad_ids_raise_before_any_launch(cases):
    c = cases["a"]
    rowptr, col = dev(c["rowptr"], c["col"])
    with pytest.raises(native.SageError, match="converge"):
        ops.pagerank(rowptr, col, max_iter=2)
    n = len(c["rowptr"]) - 1
    for bad in (-1, n, 1 << 30):
        col_bad = col.clone()
        col_bad[5] = bad
        for symmetric in (True, False):
            with pytest.raises(native.SageError, match="outside"):
                ops.pagerank(rowptr, col_bad, symmetric=symmetric)
    with pytest.raises(native.SageError, match="alpha"):
        ops.pagerank(rowptr, col, alpha=1.0)


# ---- through the stack ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def citation():
    z = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
    g = CSRGraph(z["rowptr"].astype(np.int64), z["col"].astype(np.int32), len(z["rowptr"]) - 1)
    _, labels = standin_citation(g, num_classes=7, feat_dim=16, words_per_node=2, topic_words=4)
    table = pagerank_table(g, "cuda")
    assert table.shape == (g.num_nodes, 1) and table.dtype == torch.float32 and table.is_cuda
    ref, _, _ = pagerank_fp64(g.rowptr, g.col)
    assert np.abs(table.cpu().numpy()[:, 0] - ref).sum() <= ((g.degrees() + 8) * U * ref).sum() / (1 - ALPHA)
    return g, labels.reshape(-1), table


def _losses(kind, citation):
    from sage355.exactbatch import ExactBatchTrainer
    from sage355.fullgraph import FullGraphTrainer
    from sage355.train import EngineTrainer
    g, labels, table = citation
    rowptr, col = g.to("cuda")
    lab = torch.from_numpy(labels).cuda()
    ids = torch.from_numpy(np.random.default_rng(0).permutation(g.num_nodes)[:768].astype(np.int32)).cuda().view(3, 256)
    torch.manual_seed(5)
    if kind == "full":
        tr = FullGraphTrainer(rowptr, col, table, 7, hidden1=16, hidden2=16, act1=native.ACT_SIGMOID)
        step = lambda i: tr.step(ids[i], lab[ids[i].long()])                          # noqa: E731
    elif kind == "exact":
        tr = ExactBatchTrainer(rowptr, col, table, 7, hidden1=16, hidden2=16, act1=native.ACT_SIGMOID)
        step = lambda i: tr.step(ids[i], lab[ids[i].long()])                          # noqa: E731
    else:
        tr = EngineTrainer(rowptr, col, table, 7, hidden1=16, hidden2=16, num_sample1=5, num_sample2=5, max_batch=256, act1=native.ACT_SIGMOID)
        step = lambda i: tr.step(ids[i], lab[ids[i].long()], 100 + i)                 # noqa: E731
    return torch.stack([step(i).reshape(()) for i in range(3)]).cpu()


@pytest.mark.parametrize("kind", ["full", "exact", "engine"])
def test_three_training_steps_on_the_pagerank_column(citation, kind):
    a, b = _losses(kind, citation), _losses(kind, citation)
    print(f"{kind}: losses {a.tolist()}")
    assert torch.isfinite(a).all()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_embed_all_nodes_on_the_pagerank_column_against_fp64(citation):
    from sage355.inference import embed_all_nodes
    g, _, table = citation
    rowptr, col = g.to("cuda")
    gen = torch.Generator().manual_seed(3)
    w1, w2 = torch.randn(10, 1, generator=gen) * 40, torch.randn(6, 10, generator=gen) / 3
    out = embed_all_nodes(rowptr, col, table, w1.cuda(), w2.cuda(), act1=native.ACT_SIGMOID, nan_empty=False)
    rows = torch.from_numpy(np.repeat(np.arange(g.num_nodes), g.degrees()))
    nbr = torch.from_numpy(g.col.astype(np.int64))
    cnt = torch.from_numpy(np.maximum(g.degrees(), 1)).double().unsqueeze(1)

    def mean(t):
        return torch.zeros(g.num_nodes, t.shape[1], dtype=torch.float64).index_add_(0, rows, t[nbr]) / cnt

    h1 = torch.sigmoid(mean(table.cpu().double()) @ w1.double().t())
    ref = torch.relu(mean(h1) @ w2.double().t())
    assert_close_rowmax(out.cpu(), ref, what="pagerank column through embed_all_nodes")
