"""The native classifier head (ABI 9, sage_xent_head: model.py:59-69 scores + CrossEntropyLoss, model.py:249 their gradients) on the GPU.
The reference everywhere is fp64 torch autograd on the CPU, computed from the fp32 inputs the kernel saw.  Tolerances are the project's
own (tests/test_gpu_backward_kernels.py, tests/test_gpu_engine_train.py): |scores - ref| <= 1e-5 A with A the fp64 sum of |terms|,
|loss - ref| <= 1e-5 max(1, |ref|), max|err| / max|ref| <= 2e-5 for grad_emb and grad_w; a plain fp32 evaluation of these inputs on
the CPU stays at or under 9e-7 on every one of them."""
import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.graph import rmat_graph
from sage355.train import EngineTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = native.HEAD_RANGE_ROWS
PAD = 4
SENTINEL = -777.25


def _inputs(n, c, dim, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + 7 * n + 131 * c + dim)
    emb = torch.randn(n, dim, generator=gen)
    bound = (6.0 / (c + dim)) ** 0.5                                            # xavier_uniform_ of a [C, dim] Parameter
    w = (torch.rand(c, dim, generator=gen) * 2 - 1) * bound
    labels = torch.randint(0, c, (n,), generator=gen)
    return emb, w, labels


def _reference(emb, w, labels, scale):
    """fp64 autograd; rows whose label lies outside [0, C) are masked out of the loss."""
    c = w.shape[0]
    e = emb.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    s = e @ wd.t()
    ok = (labels >= 0) & (labels < c)
    loss = scale * torch.nn.functional.cross_entropy(s[ok], labels[ok], reduction="sum")
    if ok.any() and c > 1:
        g_emb, g_w = torch.autograd.grad(loss, (e, wd))
    else:
        g_emb, g_w = torch.zeros_like(e), torch.zeros_like(wd)
    mass = emb.double().abs() @ w.double().abs().t()
    return {"scores": s.detach(), "mass": mass, "loss": loss.item(), "grad_emb": g_emb, "grad_w": g_w, "pred": s.detach().argmax(1)}


def _run(emb, w, labels, scale=None, scores=True, pred=True, grads=True):
    """One call on padded views: emb's pad is NaN (it must not be read), the outputs' pads hold a sentinel (it must survive), grad_w and
    the whole workspace start as NaN (they are stored, never accumulated).  -> dict of CPU tensors."""
    n, dim = emb.shape
    c = w.shape[0]
    emb_w = torch.full((n, dim + PAD), float("nan"))
    emb_w[:, :dim] = emb
    emb_w = emb_w.to(DEV)
    out = {}
    if scores:
        out["scores"] = torch.full((n, c + PAD), SENTINEL, device=DEV)[:, :c]
    if grads:
        out["grad_emb"] = torch.full((n, dim + PAD), SENTINEL, device=DEV)[:, :dim]
        out["grad_w"] = torch.full((c, dim), float("nan"), device=DEV)
    ws = torch.full((ops.xent_head_workspace_bytes(n, dim, c),), 0xFF, dtype=torch.uint8, device=DEV)      # 0xFFFFFFFF: a NaN in every word
    bases = {k: v._base for k, v in out.items() if v._base is not None}
    res = ops.xent_head(emb_w[:, :dim], w.to(DEV), None if labels is None else labels.to(DEV), scale=scale, scores=scores, pred=pred,
                        grads=grads, workspace=ws, out=out)
    torch.cuda.synchronize()
    for k, base in bases.items():
        width = c if k == "scores" else dim
        assert torch.equal(base[:, width:].cpu(), torch.full((n, PAD), SENTINEL)), f"{k}: the columns past the width were written"
    return {k: v.cpu() for k, v in res.items()}


def _check(got, ref, what=("scores", "loss", "grad_emb", "grad_w", "pred")):
    if "scores" in what:
        err = ((got["scores"].double() - ref["scores"]).abs() / ref["mass"].clamp_min(1e-300)).max().item()
        print(f"scores: max |err| / A = {err:.2e}")
        assert err <= 1e-5
    if "loss" in what:
        err = abs(got["loss"].item() - ref["loss"])
        print(f"loss: {got['loss'].item():.8g} vs {ref['loss']:.8g}")
        assert err <= 1e-5 * max(1.0, abs(ref["loss"]))
    for k in ("grad_emb", "grad_w"):
        if k in what:
            top = ref[k].abs().max().item()
            if top == 0.0:
                assert not got[k].any(), f"{k}: expected exact zeros"
                continue
            err = (got[k].double() - ref[k]).abs().max().item() / top
            print(f"{k}: max |err| / max |ref| = {err:.2e}")
            assert err <= 2e-5, f"{k}: {err:.2e}"


# ---- 1. edge shapes against fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dim", [(1, 4), (2, 4), (3, 100), (7, 128), (16, 256), (64, 128)])
@pytest.mark.parametrize("n", [1, R - 1, R, R + 1, 2 * R + 1, 300])
def test_edge_shapes_match_fp64_autograd(n, c, dim):
    emb, w, labels = _inputs(n, c, dim)
    got = _run(emb, w, labels)
    ref = _reference(emb, w, labels, 1.0 / n)
    _check(got, ref)
    # pred on the rows with a clear fp64 winner: each score is within 1e-5 A of its reference, so a gap above 2e-5 max A decides
    top2 = ref["scores"].topk(min(2, c), dim=1).values
    clear = torch.ones(n, dtype=torch.bool) if c == 1 else (top2[:, 0] - top2[:, 1]) > 2e-5 * ref["mass"].max(1).values
    assert torch.equal(got["pred"].long()[clear], ref["pred"][clear])
    if c == 1:
        assert got["loss"].item() == 0.0 and not got["grad_emb"].any() and not got["grad_w"].any()


# ---- 2. large logits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,dim", [(130, 7, 32), (130, 64, 64)])
def test_large_integer_logits_stay_finite_and_exact(n, c, dim):
    gen = torch.Generator().manual_seed(c)
    emb = torch.randint(-3, 4, (n, dim), generator=gen).float()
    w = torch.randint(-4, 5, (c, dim), generator=gen).float()
    labels = torch.randint(0, c, (n,), generator=gen)
    got = _run(emb, w, labels)
    ref = _reference(emb, w, labels, 1.0 / n)
    assert ref["scores"].abs().max().item() > 88.0, "the case is meant to pass the point where expf overflows"
    assert torch.isfinite(got["loss"]).all() and torch.isfinite(got["grad_emb"]).all() and torch.isfinite(got["grad_w"]).all()
    _check(got, ref, what=("loss", "grad_emb", "grad_w"))
    assert torch.equal(got["scores"].double(), ref["scores"]), "integer scores are exact in fp32"
    exact = ref["scores"].numpy()
    assert np.array_equal(got["pred"].numpy(), np.argmax(exact, axis=1)), "ties go to the lowest index"
    top2 = np.sort(exact, axis=1)[:, -2:]
    assert (top2[:, 0] == top2[:, 1]).any(), "the case is meant to have ties for the maximum"
    # one more row whose score is NaN at one class (Inf * 0) and +-Inf elsewhere: the NaN is the maximum, as torch.argmax has it
    nan_at = c // 2
    w2 = w.clone()
    w2[:, 0] = 1.0
    w2[nan_at, 0] = 0.0
    emb2 = torch.cat([emb, emb[:1]])
    emb2[n, 0] = float("inf")
    got2 = _run(emb2, w2, None, grads=False)
    s2 = emb2.double() @ w2.double().t()
    assert torch.isnan(s2[n, nan_at]) and int(torch.isnan(s2[n]).sum()) == 1
    assert int(got2["pred"][n]) == nan_at == int(s2[n].argmax())
    assert np.array_equal(got2["pred"][:n].numpy(), np.argmax(s2[:n].numpy(), axis=1))


# ---- 3. labels out of range -------------------------------------------------------------------------------------------------------
def test_out_of_range_labels_are_masked_and_never_used_as_an_index():
    n, c, dim = 65, 7, 128
    emb, w, labels = _inputs(n, c, dim, seed=3)
    rows = [2, 40, 64]
    bad = labels.clone()
    bad[rows[0]], bad[rows[1]], bad[rows[2]] = -1, c, 1 << 40
    got = _run(emb, w, bad, scale=1.0 / n)
    ref = _reference(emb, w, bad, 1.0 / n)
    _check(got, ref)
    assert not got["grad_emb"][rows].any(), "grad_emb of a row with an invalid label must be exactly zero"
    valid = _run(emb, w, labels, scale=1.0 / n)
    keep = torch.ones(n, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(got["grad_emb"][keep], valid["grad_emb"][keep])
    assert torch.equal(got["scores"], valid["scores"]) and torch.equal(got["pred"], valid["pred"])


# ---- 4. non-finite input ----------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_row_reaches_what_depends_on_it_and_nothing_else():
    n, c, dim = 65, 7, 128
    emb, w, labels = _inputs(n, c, dim, seed=4)
    emb[3, 17] = float("nan")
    got = _run(emb, w, labels)
    assert torch.isnan(got["loss"]).all()
    assert torch.isnan(got["grad_emb"][3]).all()
    others = torch.ones(n, dtype=torch.bool)
    others[3] = False
    assert torch.isfinite(got["grad_emb"][others]).all()
    assert torch.isnan(got["grad_w"]).all()
    assert torch.isnan(got["scores"][3]).all() and torch.isfinite(got["scores"][others]).all()


# ---- 5. bits ----------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_rows_do_not_depend_on_n_and_partials_add_in_range_order():
    c, dim = 7, 128
    emb, w, labels = _inputs(300, c, dim, seed=5)
    scale = 1.0 / 300
    a, b = _run(emb, w, labels, scale=scale), _run(emb, w, labels, scale=scale)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two calls on the same inputs differ"
    short = _run(emb[:65], w, labels[:65], scale=scale)
    for k in ("scores", "pred", "grad_emb"):
        assert torch.equal(short[k], a[k][:65]), f"{k}: rows [0, 65) depend on the number of rows"
    both = _run(emb[:2 * R], w, labels[:2 * R], scale=scale)
    lo = _run(emb[:R], w, labels[:R], scale=scale)
    hi = _run(emb[R:2 * R], w, labels[R:2 * R], scale=scale)
    assert torch.equal(both["grad_w"], lo["grad_w"] + hi["grad_w"]), "grad_w is not the ranges' partials added in range order"


# ---- 6. shards --------------------------------------------------------------------------------------------------------------------
def test_two_shards_at_the_global_scale_sum_to_the_full_batch():
    n, c, dim = 256, 7, 128
    emb, w, labels = _inputs(n, c, dim, seed=6)
    full = _run(emb, w, labels, scale=1.0 / n)
    lo = _run(emb[:128], w, labels[:128], scale=1.0 / n)
    hi = _run(emb[128:], w, labels[128:], scale=1.0 / n)
    for k in ("loss", "grad_w"):
        err = (lo[k] + hi[k] - full[k]).abs().max().item() / full[k].abs().max().item()
        assert err <= 1e-5, f"{k}: {err:.2e}"


# ---- 7. inference form ------------------------------------------------------------------------------------------------------------
def test_inference_form_has_the_training_forms_bits_and_refuses_gradients():
    n, c, dim = 130, 16, 64
    emb, w, labels = _inputs(n, c, dim, seed=7)
    train = _run(emb, w, labels)
    infer = _run(emb, w, None, grads=False)
    assert set(infer) == {"scores", "pred"}
    assert torch.equal(infer["scores"], train["scores"]) and torch.equal(infer["pred"], train["pred"])
    with pytest.raises(native.SageError):
        ops.xent_head(emb.to(DEV), w.to(DEV), None, grads=True)
    L = native.lib()
    e, wd = emb.to(DEV), w.to(DEV)
    g = torch.empty(c, dim, device=DEV)
    ws = torch.empty(ops.xent_head_workspace_bytes(n, dim, c), dtype=torch.uint8, device=DEV)
    rc = L.sage_xent_head(native.ptr(e), dim, dim, native.ptr(wd), dim, c, None, n, 1.0, None, 0, None, None, None, 0, native.ptr(g), dim,
                          native.ptr(ws), ws.numel(), native.stream_handle())
    assert rc == native.EINVAL


# ---- 8. the trainer with head="native" --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_graph():
    graph = rmat_graph(13, 150_000, seed=4, accel=None)
    rowptr, col = graph.to(DEV)
    return graph, rowptr, col, np.nonzero(graph.degrees() > 0)[0]


def _table(graph, d0):
    return torch.randn(graph.num_nodes, d0, generator=torch.Generator().manual_seed(1)).to(DEV)


def _autograd_reference(tr, seeds, labels):
    """fp64 torch autograd of the reference's expression (aggregators.py:54-74 mean, encoders.py:49-62 concat + W.x + relu,
    model.py:59-69 classifier + CrossEntropy) on the sets the engine sampled: the helper of tests/test_gpu_engine_train.py."""
    e = tr.engine
    it = e.intermediates()
    nbr2, cnt2, row2 = (it[k].cpu().long() for k in ("nbr2", "cnt2", "row2"))
    nbr1, cnt1 = it["nbr1"].cpu().long(), it["cnt1"].cpu().long()
    s1 = it["s1_nodes"].cpu().long()
    table = e.table[:, :e.d0].cpu().double()
    w1 = tr.w1.detach().cpu().double().requires_grad_(True)
    w2 = tr.w2.detach().cpu().double().requires_grad_(True)
    wc = tr.w_cls.detach().cpu().double().requires_grad_(True)

    def mean_rows(src, idx, cnt):
        m = (torch.arange(idx.shape[1])[None, :] < cnt[:, None]).double()
        return (src[idx.clamp_min(0)] * m[:, :, None]).sum(1) / cnt[:, None].double()

    agg1 = mean_rows(table, nbr1, cnt1)
    x1 = torch.cat([table[s1], agg1], 1) if tr.concat else agg1
    h1 = torch.relu(x1 @ w1.t())
    agg2 = mean_rows(h1, row2, cnt2)
    x2 = torch.cat([h1[:len(seeds)], agg2], 1) if tr.concat else agg2
    out = torch.relu(x2 @ w2.t())
    loss = torch.nn.functional.cross_entropy(out @ wc.t(), labels.cpu())
    g = torch.autograd.grad(loss, (w1, w2, wc))
    return loss.item(), g


def _trainer(small_graph, table, head, gcn=True, h1=128, hidden2=64, max_batch=300, lr=0.7, seed=3):
    _, rowptr, col, _ = small_graph
    torch.manual_seed(seed)
    return EngineTrainer(rowptr, col, table, 5, hidden1=h1, hidden2=hidden2, num_sample1=7, num_sample2=9, gcn=gcn, max_batch=max_batch, lr=lr,
                         head=head)


@pytest.mark.parametrize("gcn,d0,h1", [(True, 256, 128), (False, 100, 52)])
def test_native_head_step_gradients_match_fp64_autograd_on_the_same_sets(small_graph, gcn, d0, h1):
    graph, _, _, cand = small_graph
    tr = _trainer(small_graph, _table(graph, d0), "native", gcn=gcn, h1=h1)
    seeds = np.random.default_rng(2).choice(cand, 300, replace=False)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 5, 300)).to(DEV)
    loss, grads = tr.grads(torch.from_numpy(seeds.astype(np.int32)).to(DEV), labels, key=11)
    ref_loss, ref = _autograd_reference(tr, seeds, labels)
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    for name, g, r in zip(("w1", "w2", "w_cls"), grads, ref):
        err = (g.cpu().double() - r).abs().max().item() / r.abs().max().item()
        print(f"grad {name}: max |g - ref| / max|ref| = {err:.2e}")
        assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"


def test_native_and_torch_heads_agree_on_one_step(small_graph):
    graph, _, _, cand = small_graph
    table = _table(graph, 256)
    seeds = torch.from_numpy(np.random.default_rng(2).choice(cand, 300, replace=False).astype(np.int32)).to(DEV)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 5, 300)).to(DEV)
    res = {}
    for head in ("native", "torch"):
        tr = _trainer(small_graph, table, head)
        loss, grads = tr.grads(seeds, labels, key=11)
        res[head] = (loss.item(), [g.clone() for g in grads])
    assert abs(res["native"][0] - res["torch"][0]) <= 1e-5 * max(1.0, abs(res["torch"][0]))
    for name, a, b in zip(("w1", "w2", "w_cls"), res["native"][1], res["torch"][1]):
        err = (a - b).abs().max().item() / b.abs().max().item()
        assert err <= 2e-5, f"grad {name}: native vs torch head {err:.2e}"


def test_captured_native_step_trains_like_the_eager_one_and_predicts(small_graph):
    graph, rowptr, col, cand = small_graph
    table = _table(graph, 128)
    labels_by_node = torch.from_numpy(np.random.default_rng(3).integers(0, 5, graph.num_nodes)).to(DEV)
    ring = torch.from_numpy(np.stack([np.random.default_rng(10 + i).choice(cand, 256, replace=False) for i in range(4)]).astype(np.int32)).to(DEV)
    keys = [101, 102, 103, 104]

    def make():
        return _trainer(small_graph, table, "native", h1=64, hidden2=32, max_batch=256, lr=0.3, seed=5)

    eager = make()
    eager_losses = []
    for i in range(6):
        j = i % 4
        eager_losses.append(float(eager.step(ring[j], labels_by_node[ring[j].long()], keys[j])))
    cap = make()
    loss = cap.capture_step(ring, keys, labels_by_node)
    for a, b in zip(cap.parameters(), make().parameters()):
        assert torch.equal(a, b)                                 # capture (and its warm-up step) left the weights alone
    cap_losses = []
    for i in range(6):
        cap.replay_step()
        cap_losses.append(float(loss))
    assert cap_losses == eager_losses, (cap_losses, eager_losses)
    assert all(np.isfinite(cap_losses)) and cap_losses[-1] < cap_losses[0]
    for name, a, b in zip(("w1", "w2", "w_cls"), cap.parameters(), eager.parameters()):
        assert torch.equal(a, b), f"{name}: captured vs eager differ by {(a - b).abs().max().item():.3e} at {int((a != b).sum())} elements"
    # predict = the inference form on the same embeddings; rows whose two best fp64 scores are closer than 1e-4 of the largest score may
    # round either way between the kernel's FMA chain and the BLAS behind scores()
    val = torch.from_numpy(np.random.default_rng(77).choice(cand, 200, replace=False).astype(np.int32)).to(DEV)
    pred = cap.predict(val, key=5)
    assert pred.dtype == torch.int32 and pred.shape == (200,)
    s64 = cap.embed(val, key=5).cpu().double() @ cap.w_cls.cpu().double().t()
    top2 = s64.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4 * s64.abs().max().item()
    print(f"rows with a clear winner: {int(clear.sum())} of 200")
    assert int((~clear).sum()) <= 2, "more than 1 % of the rows have no clear fp64 winner: pick another seed"
    assert torch.equal(pred.cpu().long()[clear], cap.scores(val, key=5).argmax(1).cpu()[clear])
    assert torch.equal(pred.cpu().long()[clear], s64.argmax(1)[clear])


def test_native_head_keeps_w_cls_bit_identical_at_1024_seeds(small_graph):
    """The case that made _sum_over_batch necessary for the torch head: the [C, B] x [B, H2] reduction at B >= 1024."""
    graph, _, _, cand = small_graph
    table = _table(graph, 128)
    labels_by_node = torch.from_numpy(np.random.default_rng(3).integers(0, 5, graph.num_nodes)).to(DEV)
    batches = [torch.from_numpy(np.random.default_rng(20 + i).choice(cand, 1024, replace=False).astype(np.int32)).to(DEV) for i in range(3)]
    runs = []
    for _ in range(2):
        tr = _trainer(small_graph, table, "native", h1=64, hidden2=64, max_batch=1024, lr=0.3, seed=5)
        for i, ids in enumerate(batches):
            tr.step(ids, labels_by_node[ids.long()], key=200 + i)
        runs.append([w.clone() for w in tr.parameters()])
    for name, a, b in zip(("w1", "w2", "w_cls"), *runs):
        assert torch.equal(a, b), f"{name}: two runs of one schedule differ at {int((a != b).sum())} elements"
        assert torch.isfinite(a).all()


def test_native_head_refuses_an_unsupported_width_at_construction(small_graph):
    graph = small_graph[0]
    with pytest.raises(native.SageError):
        _trainer(small_graph, _table(graph, 64), "native", h1=32, hidden2=130)
