"""One exact mini-batch step (exactbatch.ExactBatchTrainer) beside one whole-graph step on the same ids (fullgraph.FullGraphTrainer)
at configs[2]'s size.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph; table 256 wide, h1 = h2 = 128, 16
classes, 4096 training ids drawn without replacement, gcn and concat encoders.  Both trainers start from one torch seed.  One
process; the two steps ALTERNATE inside one timed loop (other people's work shares the machine: a drift hits both sides alike).
Times: device events around step(), which includes the batch step's two host reads; median / min / max of --reps after --warmup.
  step     ExactBatchTrainer.step against FullGraphTrainer.step, and that their first losses are bit-equal
  memory   peak allocated bytes of one step of each above what the trainer holds between steps, and what each trainer holds
Run on an MI355X: python experiments/mb_exact_batch.py [--scale 20 --edges 16000000 --seeds 4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd"), os.path.join(REPO, "experiments")]

from mb_embed_nodes import ms, timed_pair  # noqa: E402
from sage355.exactbatch import ExactBatchTrainer  # noqa: E402
from sage355.fullgraph import FullGraphTrainer  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402


def step_peak(fn):
    """Peak allocated bytes of one call above what is allocated before it (the trainer's persistent buffers stay where they are)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_exact_batch needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0)
    n, h = g.num_nodes, args.hidden
    rp, cl = g.to("cuda")
    table = torch.randn(n, args.dim, generator=torch.Generator().manual_seed(0)).cuda()
    rs = np.random.default_rng(0)
    ids = torch.from_numpy(rs.choice(n, args.seeds, replace=False).astype(np.int32)).cuda()
    tgt = torch.from_numpy(rs.integers(0, args.classes, args.seeds)).cuda()
    shape = {"graph": f"rmat({args.scale}, {args.edges})", "nodes": n, "nnz": g.nnz, "seeds": args.seeds, "d0": args.dim, "h1": h, "h2": h,
             "classes": args.classes}
    for gcn in (True, False):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(0)
        batch = ExactBatchTrainer(rp, cl, table, args.classes, hidden1=h, hidden2=h, gcn=gcn, lr=0.05)
        first_batch = batch.step(ids, tgt).clone()
        held_batch = torch.cuda.memory_allocated() - base
        torch.manual_seed(0)
        full = FullGraphTrainer(rp, cl, table, args.classes, hidden1=h, hidden2=h, gcn=gcn, lr=0.05)
        first_full = full.step(ids, tgt).clone()
        held_full = torch.cuda.memory_allocated() - base - held_batch
        same = bool(torch.equal(first_batch.view(torch.int32), first_full.view(torch.int32)))
        tb, tf = timed_pair(lambda: batch.step(ids, tgt), lambda: full.step(ids, tgt), args.warmup, args.reps)
        enc = "gcn" if gcn else "concat"
        print(json.dumps({"case": "step", "encoder": enc, **shape, "first_loss_bit_equal": same, "exact_batch_step": ms(tb),
                          "full_graph_step": ms(tf), "batch_over_full": round(tb[0] / tf[0], 3)}), flush=True)
        print(json.dumps({"case": "memory", "encoder": enc, **shape,
                          "step_peak_MiB_exact_batch": round(step_peak(lambda: batch.step(ids, tgt)) / 2 ** 20, 1),
                          "step_peak_MiB_full_graph": round(step_peak(lambda: full.step(ids, tgt)) / 2 ** 20, 1),
                          "held_MiB_exact_batch": round(held_batch / 2 ** 20, 1), "held_MiB_full_graph": round(held_full / 2 ** 20, 1)}), flush=True)
        del batch, full


if __name__ == "__main__":
    main()
