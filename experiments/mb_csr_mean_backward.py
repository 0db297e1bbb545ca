"""csr_mean backward (sage_csr_mean_backward) against the forward (sage_csr_mean), and the whole-graph training step
(sage355.fullgraph.FullGraphTrainer) beside an epoch of sampled steps (sage355.train.EngineTrainer).

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph (30.0 M CSR entries over 1,048,576
nodes); it is symmetric, so its transpose is the graph itself with sorted rows and the two kernels move the same bytes.
  csr_mean_backward   widths 128 and 256: forward and backward in ONE process, alternating, device events around each call, median
                      of --reps; the ratio backward / forward and the rate on ALGORITHMIC bytes (every CSR entry's row + col +
                      rowptr + out; the backward also reads a 4-byte weight per entry and writes the 8 bytes per node of its pre-pass)
  fullgraph_step      FullGraphTrainer.step at configs[2]'s size (d0 256, h1 = h2 = 128, 16 classes, 80 % training rows) and on the
                      stand-in Cora (tests/golden/cora_topology.npz, 1433 -> 50 -> 128, 7 classes): --step-reps repetitions of
                      --steps steps each, median and range of the per-step time
  engine_epoch        the same split as an epoch of EngineTrainer steps of 4096 seeds (fanout 15 / 25), same box, same process
Run on an MI355X: python experiments/mb_csr_mean_backward.py [--scale 20 --edges 16000000] [--skip-train]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]

from sage355 import ops  # noqa: E402
from sage355.datasets import standin_citation  # noqa: E402
from sage355.fullgraph import FullGraphTrainer  # noqa: E402
from sage355.graph import CSRGraph, rmat_graph  # noqa: E402
from sage355.train import EngineTrainer  # noqa: E402


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def stats(ts):
    return {"ms": round(float(np.median(ts)) * 1e3, 3), "ms_min": round(float(np.min(ts)) * 1e3, 3), "ms_max": round(float(np.max(ts)) * 1e3, 3)}


def mean_bytes(n, nnz, dim):
    return nnz * (4 * dim + 4) + (n + 1) * 8 + n * 4 * dim


def kernels(g, rp, cl, rp_t, c_t, args):
    n, nnz = g.num_nodes, g.nnz
    for dim in (128, 256):
        gen = torch.Generator().manual_seed(dim)
        x = torch.randn(n, dim, generator=gen).cuda()
        out = torch.empty(n, dim, device="cuda")
        gt = torch.empty(n, dim, device="cuda")
        ws_f = torch.empty(ops.csr_mean_workspace_bytes(n, nnz, dim), dtype=torch.uint8, device="cuda")
        ws_b = torch.empty(ops.csr_mean_backward_workspace_bytes(n, n, nnz, dim), dtype=torch.uint8, device="cuda")

        def fwd():
            ops.csr_mean(rp, cl, x, out=out, workspace=ws_f)

        for self_loop in (False, True):
            def bwd():
                ops.csr_mean_backward(rp, cl, rp_t, c_t, x, self_loop=self_loop, out=gt, workspace=ws_b)

            for _ in range(args.warmup):
                fwd()
                bwd()
            torch.cuda.synchronize()
            tf, tb = [], []
            for _ in range(args.reps):                                  # alternating: both see the same state of the box
                tf.append(event_time(fwd))
                tb.append(event_time(bwd))
            by = mean_bytes(n, nnz, dim)
            by_b = by + nnz * 4 + n * 8
            f, b = float(np.median(tf)), float(np.median(tb))
            print(json.dumps({"case": "csr_mean_backward", "dim": dim, "self_loop": self_loop, "nodes": n, "nnz": nnz,
                              "forward": dict(stats(tf), TBps=round(by / f / 1e12, 2)),
                              "backward": dict(stats(tb), TBps=round(by_b / b / 1e12, 2)), "ratio": round(b / f, 3)}), flush=True)
        del x, out, gt, ws_f, ws_b
        torch.cuda.empty_cache()


def step_times(tr, ids, tgt, steps, reps):
    for _ in range(3):
        tr.step(ids, tgt)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step(ids, tgt)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps)
    return ts


def training(g, rp, cl, args):
    n = g.num_nodes
    rs = np.random.default_rng(1)
    train = rs.permutation(n)[int(0.2 * n):]
    labels = torch.from_numpy(rs.integers(0, 16, n)).cuda()
    table = torch.randn(n, 256, generator=torch.Generator(device="cuda").manual_seed(0), device="cuda")
    ids = torch.from_numpy(train.astype(np.int32)).cuda()
    for gcn in (True, False):
        torch.manual_seed(0)
        tr = FullGraphTrainer(rp, cl, table, 16, hidden1=128, hidden2=128, gcn=gcn, lr=0.05)
        ts = step_times(tr, ids, labels[ids.long()], args.steps, args.step_reps)
        print(json.dumps(dict({"case": "fullgraph_step", "graph": f"rmat({args.scale}, {args.edges})", "encoder": "gcn" if gcn else "concat",
                               "nodes": n, "train_rows": len(train), "d0": 256, "h1": 128, "h2": 128, "steps": args.steps,
                               "reps": args.step_reps}, **stats(ts))), flush=True)
        del tr
        torch.cuda.empty_cache()
    # the same training set as one epoch of sampled 4096-seed steps
    torch.manual_seed(0)
    tr = EngineTrainer(rp, cl, table, 16, hidden1=128, hidden2=128, num_sample1=15, num_sample2=25, gcn=True, lr=0.05, max_batch=4096,
                       relabel="degree")
    batches = [ids[lo:lo + 4096].contiguous() for lo in range(0, len(train), 4096)]
    tgts = [labels[b.long()] for b in batches]
    ts = []
    for rep in range(args.step_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (b, t) in enumerate(zip(batches, tgts)):
            tr.step(b, t, key=1000 * rep + i)
        torch.cuda.synchronize()
        if rep:                                                          # the first epoch is the warm-up
            ts.append(time.perf_counter() - t0)
    print(json.dumps(dict({"case": "engine_epoch", "steps_per_epoch": len(batches), "seeds_per_step": 4096, "reps": args.step_reps,
                           "ms_per_step": round(float(np.median(ts)) / len(batches) * 1e3, 4)}, **stats(ts))), flush=True)
    del tr, table
    torch.cuda.empty_cache()
    # stand-in Cora
    z = np.load(os.path.join(REPO, "tests", "golden", "cora_topology.npz"))
    cora = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
    feats, lab = standin_citation(cora, num_classes=7, feat_dim=1433, seed=0)
    crp, ccl = cora.to("cuda")
    ctrain = np.random.default_rng(1).permutation(cora.num_nodes)[int(0.2 * cora.num_nodes):]
    cids = torch.from_numpy(ctrain.astype(np.int32)).cuda()
    ctgt = torch.from_numpy(np.asarray(lab).reshape(-1)).cuda()[cids.long()]
    torch.manual_seed(0)
    tr = FullGraphTrainer(crp, ccl, torch.from_numpy(feats).cuda(), 7)
    ts = step_times(tr, cids, ctgt, 20, args.step_reps)
    print(json.dumps(dict({"case": "fullgraph_step", "graph": "standin cora", "encoder": "gcn", "nodes": cora.num_nodes,
                           "train_rows": len(ctrain), "d0": 1433, "h1": 50, "h2": 128, "steps": 20, "reps": args.step_reps}, **stats(ts))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_csr_mean_backward needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0, cache_dir=os.environ.get("SAGE_CACHE", "/tmp/sage_cache"))
    rp, cl = g.to("cuda")
    t0 = time.perf_counter()
    rp_t, c_t = ops.csr_transpose(rp, cl)
    torch.cuda.synchronize()
    print(json.dumps({"case": "csr_transpose", "nodes": g.num_nodes, "nnz": g.nnz, "ms_first_call": round((time.perf_counter() - t0) * 1e3, 1),
                      "symmetric": bool(torch.equal(rp_t, rp))}), flush=True)
    kernels(g, rp, cl, rp_t, c_t, args)
    del rp_t, c_t
    if not args.skip_train:
        training(g, rp, cl, args)


if __name__ == "__main__":
    main()
