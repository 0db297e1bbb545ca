"""The batch adjoint of the indexed CSR mean (ops.csr_mean_backward_rows, sage_csr_mean_backward_rows) at configs[2]'s size.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph; 4096 seeds drawn without
replacement, their frontier from ops.csr_frontier, the gradient of the seeds' means [4096, 128] (layer 2 reads h1, 128 wide).
One process; the two sides of every comparison ALTERNATE call by call inside one timed loop (other people's work shares the
machine: a drift hits both sides alike).  Times: device events around the call; median / min / max of --reps after --warmup.
  index_add    the kernel against the stock formulation of the same sum: the seeds' CSR ranges expanded with repeat_interleave, the
               neighbours' rows looked up in the map, zeros(|F|, dim).index_add_(rows, w * g) -- float atomics, not reproducible.
               Timed twice: with the expansion (what a caller without this kernel runs per batch) and the index_add_ alone on
               lists built beforehand.  Both sides are given E_sel.  Also: the largest difference between the two results.
  whole_graph  the kernel against what the tree offered before it: the seeds' gradient rows scattered into [N, dim] and
               ops.csr_mean_backward over every node (its transpose built once, outside the timing)
  memory       peak allocated bytes above the inputs of one call of each
Run on an MI355X: python experiments/mb_csr_mean_backward_rows.py [--scale 20 --edges 16000000 --seeds 4096 --dim 128]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd"), os.path.join(REPO, "experiments")]

from mb_embed_nodes import ms, peak_of, timed_pair  # noqa: E402
from sage355 import ops  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_csr_mean_backward_rows needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0)
    n, dim, m = g.num_nodes, args.dim, args.seeds
    rp, cl = g.to("cuda")
    seeds = torch.from_numpy(np.random.default_rng(0).choice(n, m, replace=False).astype(np.int32)).cuda()
    s64 = seeds.long()
    e_sel = int((rp[s64 + 1] - rp[s64]).sum())
    fr = ops.CsrFrontier(n, "cuda", max_nodes=min(n, m + e_sel))
    ops.csr_frontier(rp, cl, seeds, fr, max_edges=e_sel)
    rows = fr.size()
    pos = fr.pos
    grad = torch.randn(m, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    shape = {"graph": f"rmat({args.scale}, {args.edges})", "nodes": n, "nnz": g.nnz, "seeds": m, "seed_edges": e_sel, "frontier": rows, "dim": dim}
    ws = torch.empty(ops.csr_mean_backward_rows_workspace_bytes(m, e_sel, rows, dim), dtype=torch.uint8, device="cuda")
    out = torch.empty(rows, dim, device="cuda")

    def kernel():
        return ops.csr_mean_backward_rows(rp, cl, seeds, grad, index=pos, num_rows=rows, out=out, max_edges=e_sel, workspace=ws)

    def expand():
        start = rp[s64]
        deg = rp[s64 + 1] - start
        first = torch.cumsum(deg, 0) - deg
        idx = torch.repeat_interleave(start - first, deg, output_size=e_sel) + torch.arange(e_sel, device="cuda")
        src = torch.repeat_interleave(torch.arange(m, device="cuda"), deg, output_size=e_sel)
        w = torch.where(deg > 0, 1.0 / deg.clamp_min(1).float(), torch.zeros((), device="cuda"))
        return pos[cl[idx].long()].long(), src, w

    def stock(lists=None):
        keys, src, w = expand() if lists is None else lists
        return torch.zeros(rows, dim, device="cuda").index_add_(0, keys, grad[src] * w[src, None])

    lists = expand()
    got, ref = kernel().clone(), stock(lists)
    diff = float((got - ref).abs().max() / ref.abs().max())
    again = bool(torch.equal(kernel().view(torch.int32), got.view(torch.int32)))
    tk, ts = timed_pair(kernel, stock, args.warmup, args.reps)
    tk2, ta = timed_pair(kernel, lambda: stock(lists), args.warmup, args.reps)
    print(json.dumps({"case": "index_add", **shape, "max_diff_over_max": diff, "kernel_bit_equal_twice": again, "csr_mean_backward_rows": ms(tk),
                      "expand_and_index_add": ms(ts), "kernel_over_stock": round(tk[0] / ts[0], 3), "csr_mean_backward_rows_2": ms(tk2),
                      "index_add_alone": ms(ta), "kernel_over_index_add_alone": round(tk2[0] / ta[0], 3)}), flush=True)

    rp_t, c_t = ops.csr_transpose(rp, cl)
    ws_all = torch.empty(ops.csr_mean_backward_workspace_bytes(n, n, c_t.numel(), dim), dtype=torch.uint8, device="cuda")

    def whole():
        scattered = torch.zeros(n, dim, device="cuda").index_copy_(0, s64, grad)
        return ops.csr_mean_backward(rp, cl, rp_t, c_t, scattered, workspace=ws_all)

    by_node = whole()[fr.nodes[:rows].long()]
    diff_all = float((got - by_node).abs().max() / by_node.abs().max())
    tk3, tw = timed_pair(kernel, whole, args.warmup, max(5, args.reps // 2))
    print(json.dumps({"case": "whole_graph", **shape, "max_diff_over_max": diff_all, "csr_mean_backward_rows": ms(tk3),
                      "scatter_and_csr_mean_backward": ms(tw), "kernel_over_whole_graph": round(tk3[0] / tw[0], 3)}), flush=True)

    print(json.dumps({"case": "memory", **shape, "workspace_MiB": round(ws.numel() / 2 ** 20, 2),
                      "peak_MiB_kernel_own_workspace": round(peak_of(lambda: ops.csr_mean_backward_rows(rp, cl, seeds, grad, index=pos, num_rows=rows,
                                                                                                          max_edges=e_sel)) / 2 ** 20, 2),
                      "peak_MiB_expand_and_index_add": round(peak_of(stock) / 2 ** 20, 2),
                      "peak_MiB_scatter_and_csr_mean_backward": round(peak_of(whole) / 2 ** 20, 2)}), flush=True)


if __name__ == "__main__":
    main()
