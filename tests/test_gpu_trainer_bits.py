"""The BITS of the three trainers (train.EngineTrainer, fullgraph.FullGraphTrainer, exactbatch.ExactBatchTrainer) and of their run
drivers, pinned: tests/golden/trainer_bits.json maps a case name to SHA-256 digests of `start` -- the parameters straight after
construction -- and of `end` -- the stacked losses of three steps and the parameters after them (a driver case: its losses and its
trainer's final parameters, `end` alone).

The neighbouring tests hold every trainer to fp64 within a bound and check that two runs give the same bits; none of them would
notice another reduction form in the head, another draw order of the weights, another batch boundary or another key sequence that
stays inside the bound.  This one does.  A change of torch's generators shows in `start` as well; a change of the code in `end` alone.

The digests were recorded from the sage355 package of commit afe62c9 ("Train on exact mini-batches: batch adjoint of the indexed CSR
mean"), the last one in which each trainer carried its own copy of the head, of the weight start and of the batch loop; the recording
was made twice and the two files were identical.

Inputs are tests/test_gpu_exact_batch_train.py's: rmat_graph(11, 30_000, seed=4) -- 2048 nodes, a hub above CSR_MEAN_CHUNK, isolated
nodes --, 300 distinct ids and their labels from default_rng(2), 5 classes, a CPU-generated table of width 64, hidden1 = 32,
hidden2 = 64, torch.manual_seed immediately before every construction.  The drivers run on standin_citation(graph, 7, 64, seed=0).
The sampled trainer keeps the reference's rule that a seed without neighbours gives NaN (0 / 0, aggregators.py:63), and one NaN loss
turns every weight into NaN for good -- bits that pin nothing.  So EngineTrainer's 300 ids are drawn from the nodes that have
neighbours, as tests/test_gpu_engine_train.py draws them, and its driver, which trains on every node, runs on the Cora topology of
tests/golden (no isolated node); every case requires its losses to be finite.

To record (only ever from the package of the commit BEFORE a change that must keep the bits, with this build's library; PATH
defaults to the golden file; record twice and keep the file only if the two are identical):
    SAGE355_LIB=<libsage355.so> PYTHONPATH=<that commit's graphsage-simple_amd>:tests python tests/test_gpu_trainer_bits.py --record [PATH]"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from sage355 import native
from sage355.datasets import standin_citation
from sage355.exactbatch import ExactBatchTrainer, run_exact_batch_training
from sage355.fullgraph import FullGraphTrainer, degree_index, run_full_graph_training
from sage355.graph import CSRGraph, rmat_graph
from sage355.train import EngineTrainer, run_engine_training
from test_gpu_chunked_sum_bits import digest

DEV = "cuda"
CLASSES, TRAIN, STEPS, SEED = 5, 300, 3, 3
SIZES = dict(hidden1=32, hidden2=64)
KEYS = (100, 101, 102)                                            # the sampler keys of the EngineTrainer cases' three steps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_bits.json")

_setup = {}


def setup():
    if not _setup:
        graph = rmat_graph(11, 30_000, seed=4, accel=None)
        deg = graph.degrees()
        assert graph.num_nodes == 2048 and int(deg.max()) > native.CSR_MEAN_CHUNK and int((deg == 0).sum()) > 0
        rs = np.random.default_rng(2)
        ids = rs.choice(graph.num_nodes, TRAIN, replace=False)
        labels = torch.from_numpy(rs.integers(0, CLASSES, TRAIN))
        linked = np.random.default_rng(2).choice(np.nonzero(deg > 0)[0], TRAIN, replace=False)
        z = np.load(os.path.join(os.path.dirname(GOLDEN), "cora_topology.npz"))
        cora = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
        rowptr, col = graph.to(DEV)
        index, rows = degree_index(rowptr)
        _setup.update(graph=graph, rowptr=rowptr, col=col, ids=torch.from_numpy(ids.astype(np.int32)).to(DEV), labels=labels.to(DEV),
                      table=torch.randn(graph.num_nodes, 64, generator=torch.Generator().manual_seed(64)).to(DEV),
                      embed=dict(embed_index=index, embed_rows=rows, embed_dim=8, act1=native.ACT_SIGMOID),
                      linked=torch.from_numpy(linked.astype(np.int32)).to(DEV), graph_standin=standin_citation(graph, 7, 64, seed=0),
                      cora=cora, cora_standin=standin_citation(cora, 7, 64, seed=0))
    return _setup


def trainer_case(build, step):
    """build(setup) -> a trainer, step(trainer, setup, i) -> the loss of step i."""
    def run():
        s = setup()
        torch.manual_seed(SEED)
        tr = build(s)
        start = digest(*tr.parameters())
        losses = torch.stack([step(tr, s, i).reshape(()) for i in range(STEPS)])       # stacked at once: a loss may live in a buffer
        assert bool(torch.isfinite(losses).all()), losses                               # of the trainer that its next step rewrites
        return {"start": start, "end": digest(losses, *tr.parameters())}
    return run


def engine_case(table, **kw):
    return trainer_case(lambda s: EngineTrainer(s["rowptr"], s["col"], s["table"] if table else None, CLASSES, num_sample1=5, num_sample2=5,
                                                max_batch=TRAIN, **SIZES, **({} if table else s["embed"]), **kw),
                        lambda tr, s, i: tr.step(s["linked"], s["labels"], KEYS[i]).clone())


def full_case(table, **kw):
    return trainer_case(lambda s: FullGraphTrainer(s["rowptr"], s["col"], s["table"] if table else None, CLASSES, **SIZES,
                                                   **({} if table else s["embed"]), **kw),
                        lambda tr, s, i: tr.step(s["ids"], s["labels"]).clone())


def exact_case(**kw):
    return trainer_case(lambda s: ExactBatchTrainer(s["rowptr"], s["col"], s["table"], CLASSES, **SIZES, **kw),
                        lambda tr, s, i: tr.step(s["ids"], s["labels"]).clone())


def driver_case(driver, graph="graph", **kw):
    def run():
        s = setup()
        feats, labels = s[graph + "_standin"]
        torch.manual_seed(SEED)
        res = driver(s[graph], feats, labels, 7, seed=1, **kw)
        assert len(res["losses"]) >= 3 and bool(np.isfinite(res["losses"]).all()), res["losses"]
        return {"end": digest(torch.tensor(res["losses"], dtype=torch.float64), *res["trainer"].parameters())}
    return run


CASES = {}
for _gcn in (True, False):
    for _head in ("native", "torch"):
        _tag = f"{'gcn' if _gcn else 'concat'}-{_head}"
        CASES[f"engine-{_tag}"] = engine_case(True, gcn=_gcn, head=_head)
        CASES[f"full-{_tag}"] = full_case(True, gcn=_gcn, head=_head)
        CASES[f"exact-{_tag}"] = exact_case(gcn=_gcn, head=_head, agg_self_loop=(not _gcn and _head == "native"))
for _sparse in (False, True):
    CASES[f"engine-embed-{'sparse' if _sparse else 'dense'}"] = engine_case(False, gcn=True, head="native", sparse_embed=_sparse)
for _gcn in (True, False):
    for _fused in (False, True):
        CASES[f"full-embed-{'gcn' if _gcn else 'concat'}-{'fused' if _fused else 'plain'}"] = full_case(False, gcn=_gcn, head="native",
                                                                                                      fused_embed=_fused)
for _ref in (False, True):
    _tag = "-ref_batching" if _ref else ""
    CASES[f"run_engine-native{_tag}"] = driver_case(run_engine_training, "cora", epochs=1, batch_size=128, ref_batching=_ref, head="native")
    CASES[f"run_exact{_tag}"] = driver_case(run_exact_batch_training, epochs=1, batch_size=128, ref_batching=_ref)
CASES["run_engine-torch"] = driver_case(run_engine_training, "cora", epochs=1, batch_size=128)
CASES["run_full"] = driver_case(run_full_graph_training, steps=3)


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded_and_nothing_else():
    assert sorted(recorded()) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_bits_are_the_recorded_ones(name):
    got, want = CASES[name](), recorded()[name]
    print(name, got)
    assert got.get("start") == want.get("start"), f"{name}: the parameters START with other bits (torch's generators, or the draw order)"
    assert got["end"] == want["end"], f"{name}: SHA-256 {got['end']} after the steps, recorded {want['end']}"


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit(__doc__)
    path = sys.argv[2] if len(sys.argv) == 3 else GOLDEN
    out = {}
    for case_name in sorted(CASES):
        out[case_name] = CASES[case_name]()
        print(case_name, out[case_name], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    import sage355
    print(f"recorded {len(out)} cases from {os.path.dirname(sage355.__file__)} ({native.LIB_PATH}) -> {path}")
