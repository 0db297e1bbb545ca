"""ops.eigen_top on the GPU against the LA.eig goldens (tests/golden/eigen_cases.npz), and datasets.eigen_table through the trainers.

Every golden case is run once, at tol = TOL = 3e-5.  All checks are computed here in fp64 from the returned fp32 block V and the
dense adjacency matrix A:  Q = qr(V),  H = Q^T A Q (eigenvalues mu_1 >= ... >= mu_k),  R = A Q - Q H.

  contract    ||A v_j - theta_j v_j||_2 <= 2 tol theta_1 for the returned (theta_j, v_j): the implementation stops on its own fp32
              evaluation of these norms; the factor 2 covers that evaluation and the last orthonormalisation.
  orthonormal the returned block is an orthonormal block rounded to fp32 ONCE (ops._round_once): V = W (1 + d), |d| <= u = 2^-24,
              W^T W = I up to the fp64 Cholesky-QR pass that made W.  So (V^T V - I)_jk = sum_i W_ij W_ik (d_ij + d_ik + d_ij d_ik)
              + (W^T W - I)_jk, and |V^T V - I|_jk <= (2 u + u^2) (|V|^T |V|)_jk / (1 - u)^2 + e64, which Cauchy-Schwarz keeps
              below 2^-23 (1.2e-7) on and off the diagonal.  e64 = 64 (N k + k (k + 1)) 2^-53 is the orthogonality bound of one
              Cholesky-QR pass on a block of condition number ~ 1 (Yamamoto, Nakatsukasa, Yanagisawa, Fukaya, ETNA 44 (2015),
              the bound of CholeskyQR2's second pass); 2e-9 at Cora's size.  The fp32 prototype of this scheme, which rotated in
              fp32 and stopped there, measured 7-9e-7.
  values      |theta_j - lambda_j| <= ||R||_F against the sorted golden eigenvalues (Kahan: the Ritz values of an orthonormal
              block lie within ||R||_2 of k distinct eigenvalues; the golden's gap lambda_k - lambda_(k+1) >= 2 sqrt(k) TOL
              lambda_1 makes a block that holds another pair than the top k a violation).
  subspace    ||(I - U U^T) Q||_2 <= ||R||_F / (mu_k - lambda_(k+1)), U the golden vectors (Davis-Kahan), the sine computed as
              written; and, for every j whose golden neighbours are more than 8 ||R||_F away, the same for column j alone against
              +-u_j with the distance of mu_j to lambda_(j-1) and lambda_(j+1) as the gap."""
import os

import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.datasets import eigen_table, standin_citation
from sage355.graph import CSRGraph
from test_eigen_host import TOL, dense_adjacency, golden_cases
from util import GOLDEN_DIR, assert_close_rowmax

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CASES = ["a", "b", "b32", "c", "cora"]


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.fixture(scope="module")
def cases():
    return golden_cases()


@pytest.fixture(scope="module")
def runs(cases):
    """Every golden case run once: (values, vectors, iterations, history) and the fp64 quantities of the docstring."""
    out = {}
    for name, c in cases.items():
        hist = []
        values, vectors, it = ops.eigen_top(*dev(c["rowptr"], c["col"]), c["k"], tol=TOL, history=hist)
        a = dense_adjacency(c["rowptr"], c["col"])
        v = vectors.cpu().numpy().astype(np.float64)
        q, _ = np.linalg.qr(v)
        aq = a @ q
        h = q.T @ aq
        h = (h + h.T) / 2
        out[name] = dict(values=values, vectors=vectors, iterations=it, history=hist, a=a, v=v, q=q, r=aq - q @ h,
                         mu=np.linalg.eigvalsh(h)[::-1])
    return out


@pytest.mark.parametrize("name", CASES)
def test_contract(cases, runs, name):
    c, r = cases[name], runs[name]
    k, n = c["k"], len(c["rowptr"]) - 1
    values, vectors, v = r["values"], r["vectors"], r["v"]
    assert values.dtype == torch.float64 and tuple(values.shape) == (k,) and not values.is_cuda
    assert vectors.dtype == torch.float32 and tuple(vectors.shape) == (n, k) and vectors.is_cuda and vectors.is_contiguous()
    assert 1 <= r["iterations"] == len(r["history"])
    theta = values.numpy()
    assert np.all(np.diff(theta) <= 0) and theta[0] > 0
    res = np.linalg.norm(r["a"] @ v - v * theta, axis=0)
    gram = v.T @ v
    bound = (2 * U + U * U) * (np.abs(v).T @ np.abs(v)) / (1 - U) ** 2 + 64 * (n * k + k * (k + 1)) * 2.0 ** -53
    orth = np.abs(gram - np.eye(k))
    print(f"case {name}: N={n} k={k} iterations={r['iterations']} max residual / (tol theta_1) = {res.max() / (TOL * theta[0]):.3f} "
          f"(own fp32 evaluation: {r['history'][-1] / (TOL * theta[0]):.3f}), max |V^T V - I| = {orth.max():.2e} "
          f"({(orth / bound).max():.3f} of its bound; the fp32 prototype: 9e-7), max | |v_j| - 1 | = {np.abs(np.sqrt(np.diag(gram)) - 1).max():.2e}")
    assert r["history"][-1] <= TOL * theta[0]
    assert np.all(res <= 2 * TOL * theta[0])
    assert np.all(orth <= bound)
    lead = np.abs(v).argmax(0)                                        # numpy: the first index of the maximum
    assert np.all(v[lead, np.arange(k)] > 0)


@pytest.mark.parametrize("name", CASES)
def test_values_and_subspace_against_the_golden(cases, runs, name):
    c, r = cases[name], runs[name]
    k, lam, u = c["k"], c["values"], c["vectors"]
    q, mu, theta = r["q"], r["mu"], r["values"].numpy()
    rf = np.linalg.norm(r["r"])
    assert np.all(np.abs(theta - lam[:k]) <= rf) and np.all(np.abs(mu - lam[:k]) <= rf)
    gap = mu[-1] - lam[k]
    assert gap > 0
    sine = np.linalg.norm(q - u @ (u.T @ q), 2)
    print(f"case {name}: ||R||_F / theta_1 = {rf / lam[0]:.2e}, max |theta - lambda| / ||R||_F = {np.abs(theta - lam[:k]).max() / rf:.3f}, "
          f"sin(subspace angle) = {sine:.2e} = {sine / (rf / gap):.3f} of ||R||_F / gap")
    assert sine <= rf / gap
    above = np.concatenate([[np.inf], lam[:k - 1]])                   # lambda_(j-1), lambda_(j+1) of every j < k
    below = lam[1:k + 1]
    checked, worst = 0, 0.0
    for j in np.nonzero(np.minimum(above - lam[:k], lam[:k] - below) > 8 * rf)[0]:
        vj = r["v"][:, j] / np.linalg.norm(r["v"][:, j])
        sj = np.linalg.norm(vj - u[:, j] * (u[:, j] @ vj))
        bj = rf / min(above[j] - mu[j], mu[j] - below[j])
        checked, worst = checked + 1, max(worst, sj / bj)
        assert sj <= bj, (j, sj, bj)
    print(f"case {name}: {checked} of {k} columns stand apart by 8 ||R||_F: max sine / bound = {worst:.3f}")
    assert checked >= 1


def test_two_runs_give_the_same_bits(cases, runs):
    for name in ("b", "cora"):
        c, r = cases[name], runs[name]
        hist = []
        values, vectors, it = ops.eigen_top(*dev(c["rowptr"], c["col"]), c["k"], tol=TOL, history=hist)
        assert it == r["iterations"] and hist == r["history"]
        assert torch.equal(values, r["values"])
        assert torch.equal(vectors.view(torch.int32), r["vectors"].view(torch.int32))


def test_failure_modes(cases):
    c = cases["cora"]
    rowptr, col = dev(c["rowptr"], c["col"])
    with pytest.raises(native.SageError, match="converge"):
        ops.eigen_top(rowptr, col, c["k"], tol=TOL, max_iter=1)
    a = cases["a"]
    rp, cl = a["rowptr"].copy(), a["col"]
    first = int(np.nonzero(np.diff(rp) > 1)[0][0])                    # drop one entry of one row: its mirror stays
    cut = np.delete(cl, rp[first])
    rp[first + 1:] -= 1
    with pytest.raises(native.SageError, match="symmetric"):
        ops.eigen_top(*dev(rp, cut), 2)
    n = len(a["rowptr"]) - 1
    with pytest.raises(native.SageError, match="k = "):
        ops.eigen_top(*dev(a["rowptr"], a["col"]), n + 1)
    with pytest.raises(native.SageError, match="no entries"):
        ops.eigen_top(*dev(np.zeros(5, dtype=np.int64), np.zeros(0, dtype=np.int32)), 2)
    bad = a["col"].copy()
    bad[3] = n
    with pytest.raises(native.SageError, match="outside"):
        ops.eigen_top(*dev(a["rowptr"], bad), 2)


def test_every_column_of_a_graph_smaller_than_the_block(cases):
    """m = min(N, k + guard) = N: the first Rayleigh-Ritz is the whole eigenproblem; no filter runs."""
    a = cases["a"]
    n = len(a["rowptr"]) - 1
    values, vectors, it = ops.eigen_top(*dev(a["rowptr"], a["col"]), n - 4, tol=TOL)
    lam = np.linalg.eigvalsh(dense_adjacency(a["rowptr"], a["col"]))[::-1]
    assert it == 1 and tuple(vectors.shape) == (n, n - 4)
    assert np.abs(values.numpy() - lam[:n - 4]).max() <= 2 * TOL * lam[0]


# ---- through the stack ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def citation():
    z = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
    g = CSRGraph(z["rowptr"].astype(np.int64), z["col"].astype(np.int32), len(z["rowptr"]) - 1)
    feat, labels = standin_citation(g, num_classes=7, feat_dim=16, words_per_node=2, topic_words=4)
    table = eigen_table(g, "cuda", 16, tol=TOL)
    assert tuple(table.shape) == (g.num_nodes, 16) and table.dtype == torch.float32 and table.is_cuda
    return g, labels, table


def _losses(kind, citation):
    from sage355.exactbatch import ExactBatchTrainer
    from sage355.fullgraph import FullGraphTrainer
    from sage355.train import run_engine_training
    g, labels, table = citation
    torch.manual_seed(5)
    if kind == "engine":                                              # the run driver takes the table as feat_data, default ReLU
        batch = -(-(g.num_nodes - int(0.2 * g.num_nodes)) // 3)       # the training share of the 10 / 10 / 80 split in three batches
        res = run_engine_training(g, table, labels, 7, epochs=1, batch_size=batch, hidden1=16, hidden2=16, num_sample1=5, num_sample2=5)
        assert len(res["losses"]) == 3
        return torch.stack([torch.as_tensor(x).reshape(()).cpu() for x in res["losses"]])
    rowptr, col = g.to("cuda")
    lab = torch.from_numpy(labels.reshape(-1)).cuda()
    ids = torch.from_numpy(np.random.default_rng(0).permutation(g.num_nodes)[:768].astype(np.int32)).cuda().view(3, 256)
    cls = FullGraphTrainer if kind == "full" else ExactBatchTrainer
    tr = cls(rowptr, col, table, 7, hidden1=16, hidden2=16)
    return torch.stack([tr.step(ids[i], lab[ids[i].long()]).reshape(()) for i in range(3)]).cpu()


@pytest.mark.parametrize("kind", ["full", "exact", "engine"])
def test_three_training_steps_on_the_eigen_table(citation, kind):
    a, b = _losses(kind, citation), _losses(kind, citation)
    print(f"{kind}: losses {a.tolist()}")
    assert a.shape == (3,) and torch.isfinite(a).all()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_embed_all_nodes_on_the_eigen_table_against_fp64(citation):
    from sage355.inference import embed_all_nodes
    g, _, table = citation
    rowptr, col = g.to("cuda")
    gen = torch.Generator().manual_seed(3)
    w1, w2 = torch.randn(10, 16, generator=gen), torch.randn(6, 10, generator=gen) / 3
    out = embed_all_nodes(rowptr, col, table, w1.cuda(), w2.cuda(), nan_empty=False)
    rows = torch.from_numpy(np.repeat(np.arange(g.num_nodes), g.degrees()))
    nbr = torch.from_numpy(g.col.astype(np.int64))
    cnt = torch.from_numpy(np.maximum(g.degrees(), 1)).double().unsqueeze(1)

    def mean(t):
        return torch.zeros(g.num_nodes, t.shape[1], dtype=torch.float64).index_add_(0, rows, t[nbr]) / cnt

    h1 = torch.relu(mean(table.cpu().double()) @ w1.double().t())
    ref = torch.relu(mean(h1) @ w2.double().t())
    assert_close_rowmax(out.cpu(), ref, what="eigen table through embed_all_nodes")
