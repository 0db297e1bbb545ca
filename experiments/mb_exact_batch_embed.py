"""Exact mini-batch steps on a TRAINABLE embedding (exactbatch.ExactBatchEmbedTrainer) at configs[2]'s size: the dense embedding
gradient against sparse_embed, and the touched-rows kernel alone against what it replaces.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph; embed_dim 256, h1 = h2 = 128, 16
classes, 4096 training ids drawn without replacement, gcn encoder.  One process; the variants of a case ALTERNATE inside one timed
loop (other people's work shares the machine: a drift hits both sides alike).  Times: device events, median / min / max of --reps
after --warmup; a step includes its two host reads.
  step     1hot: ExactBatchEmbedTrainer.step dense against sparse_embed; node_degree: dense against the frozen-table
           ExactBatchTrainer.step (context); FullGraphTrainer(embed_index=1hot).step on the same ids (context, timed alone)
  kernel   on one batch's frontier and a random layer-1 gradient: ops.csr_mean_backward_touched(table=, lr=, want_grad=False)
           against ops.csr_mean_backward_rows at num_rows = R followed by embed.add_, and against torch index_add_ on PREBUILT term
           lists (float atomics: NOT reproducible, and the lists' construction is not timed; shown for scale only)
  memory   peak allocated bytes of one step above what is allocated before it, per variant
Run on an MI355X: python experiments/mb_exact_batch_embed.py [--scale 20 --edges 16000000 --seeds 4096]
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
from mb_exact_batch import step_peak  # noqa: E402
from sage355 import ops  # noqa: E402
from sage355.exactbatch import ExactBatchEmbedTrainer, ExactBatchTrainer  # noqa: E402
from sage355.fullgraph import FullGraphTrainer, degree_index, one_hot_index  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402
from sage355.native import ACT_RELU, ACT_SIGMOID  # noqa: E402


def mib(x):
    return round(x / 2 ** 20, 1)


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
    ap.add_argument("--no-full", action="store_true", help="skip the whole-graph trainer")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_exact_batch_embed needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0)
    n, h, d, lr = g.num_nodes, args.hidden, args.dim, 0.05
    rp, cl = g.to("cuda")
    rs = np.random.default_rng(0)
    ids = torch.from_numpy(rs.choice(n, args.seeds, replace=False).astype(np.int32)).cuda()
    tgt = torch.from_numpy(rs.integers(0, args.classes, args.seeds)).cuda()
    one, deg = one_hot_index(n, "cuda"), degree_index(rp)
    shape = {"graph": f"rmat({args.scale}, {args.edges})", "nodes": n, "nnz": g.nnz, "seeds": args.seeds, "embed_dim": d, "h1": h, "h2": h,
             "classes": args.classes}
    kw = dict(hidden1=h, hidden2=h, lr=lr)

    def embed_trainer(index, rows, act1, sparse):
        torch.manual_seed(0)
        return ExactBatchEmbedTrainer(rp, cl, args.classes, index, rows, d, act1=act1, sparse_embed=sparse, **kw)

    # ---- 1hot: dense against sparse ------------------------------------------------------------------------------------------------
    dense, sparse = embed_trainer(*one, ACT_RELU, False), embed_trainer(*one, ACT_RELU, True)
    first = [t.step(ids, tgt).clone() for t in (dense, sparse)]
    td, ts = timed_pair(lambda: dense.step(ids, tgt), lambda: sparse.step(ids, tgt), args.warmup, args.reps)
    print(json.dumps({"case": "step", "initializer": "1hot", "embed_rows": one[1], **shape,
                      "first_loss_bit_equal": bool(torch.equal(first[0].view(torch.int32), first[1].view(torch.int32))),
                      "dense_step": ms(td), "sparse_step": ms(ts), "sparse_over_dense": round(ts[0] / td[0], 3)}), flush=True)
    print(json.dumps({"case": "memory", "initializer": "1hot", "embed_rows": one[1], **shape,
                      "step_peak_MiB_dense": mib(step_peak(lambda: dense.step(ids, tgt))),
                      "step_peak_MiB_sparse": mib(step_peak(lambda: sparse.step(ids, tgt))), "embed_MiB": mib(4 * one[1] * d)}), flush=True)

    # ---- the kernel alone, on this batch's frontier --------------------------------------------------------------------------------
    try:
        f = sparse._forward(ids)
        f_nodes, e1 = f["f_nodes"].clone(), f["e1"]
    finally:
        sparse.frontier.clear()
    size = f_nodes.shape[0]
    g1 = torch.randn(size, d, device="cuda")
    for name, (index, rows) in (("1hot", one), ("node_degree", deg)):
        embed = torch.randn(rows, d, device="cuda")
        ws_t = torch.empty(ops.csr_mean_backward_touched_workspace_bytes(size, e1, rows, d), dtype=torch.uint8, device="cuda")
        ws_r = torch.empty(ops.csr_mean_backward_rows_workspace_bytes(size, e1, rows, d), dtype=torch.uint8, device="cuda")
        out_t = (None, torch.empty(1, dtype=torch.int32, device="cuda"), None)
        dense_out = torch.empty(rows, d, device="cuda")

        def touched():
            ops.csr_mean_backward_touched(rp, cl, f_nodes, g1, index=index, num_rows=rows, max_edges=e1, table=embed, lr=lr, want_grad=False,
                                          out=out_t, workspace=ws_t)

        def dense_add():
            embed.add_(ops.csr_mean_backward_rows(rp, cl, f_nodes, g1, index=index, num_rows=rows, max_edges=e1, out=dense_out, workspace=ws_r),
                       alpha=-lr)

        # the prebuilt lists of the atomic form: every term's embedding row, and its weighted gradient row
        v = f_nodes.long()
        cnt = rp[v + 1] - rp[v]
        src = torch.repeat_interleave(torch.arange(size, device="cuda"), cnt)
        pos = torch.arange(int(cnt.sum()), device="cuda") - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        keys = index[cl[rp[v][src] + pos].long()].long()
        w = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1).float(), torch.zeros(size, device="cuda"))

        tt, tr_ = timed_pair(touched, dense_add, args.warmup, args.reps)
        tt2 = ta = None
        if keys.numel() * d * 4 <= 16 << 30:                           # the term rows themselves are prebuilt too: [terms, embed_dim]
            rows_w = (g1 * w[:, None])[src]
            tt2, ta = timed_pair(touched, lambda: embed.index_add_(0, keys, rows_w, alpha=-lr), args.warmup, args.reps)
            del rows_w
        print(json.dumps({"case": "kernel", "initializer": name, "embed_rows": rows, "frontier": size, "terms": e1, "touched_rows": int(out_t[1]),
                          "embed_dim": d, "touched_update": ms(tt), "backward_rows_plus_add": ms(tr_), "touched_over_rows": round(tt[0] / tr_[0], 3),
                          "touched_update_again": ms(tt2) if tt2 else "not measured",
                          "index_add_prebuilt_NOT_reproducible": ms(ta) if ta else "not measured",
                          "workspace_MiB_touched": mib(ws_t.numel()), "workspace_MiB_rows": mib(ws_r.numel())}), flush=True)
        del embed, ws_t, ws_r, dense_out, keys, src, pos
    del dense, sparse
    torch.cuda.empty_cache()

    # ---- node_degree dense, beside the frozen-table trainer (context) ---------------------------------------------------------------
    degree = embed_trainer(*deg, ACT_SIGMOID, False)
    torch.manual_seed(0)
    frozen = ExactBatchTrainer(rp, cl, torch.randn(n, d, generator=torch.Generator().manual_seed(0)).cuda(), args.classes, **kw)
    tg, tf = timed_pair(lambda: degree.step(ids, tgt), lambda: frozen.step(ids, tgt), args.warmup, args.reps)
    print(json.dumps({"case": "step", "initializer": "node_degree", "embed_rows": deg[1], **shape, "dense_step": ms(tg),
                      "frozen_table_step": ms(tf), "dense_over_frozen": round(tg[0] / tf[0], 3)}), flush=True)
    print(json.dumps({"case": "memory", "initializer": "node_degree", "embed_rows": deg[1], **shape,
                      "step_peak_MiB_dense": mib(step_peak(lambda: degree.step(ids, tgt))),
                      "step_peak_MiB_frozen_table": mib(step_peak(lambda: frozen.step(ids, tgt)))}), flush=True)
    del frozen
    torch.cuda.empty_cache()
    if args.no_full:
        return
    # ---- the whole-graph trainer on the same ids (context) ----------------------------------------------------------------------------
    torch.manual_seed(0)
    full = FullGraphTrainer(rp, cl, None, args.classes, embed_index=one[0], embed_rows=one[1], embed_dim=d, **kw)
    tg, tw = timed_pair(lambda: degree.step(ids, tgt), lambda: full.step(ids, tgt), 1, max(args.reps // 4, 3))
    print(json.dumps({"case": "step", "initializer": "1hot", "embed_rows": one[1], **shape, "full_graph_step": ms(tw),
                      "step_peak_MiB_full_graph": mib(step_peak(lambda: full.step(ids, tgt)))}), flush=True)


if __name__ == "__main__":
    main()
