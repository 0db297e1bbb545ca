"""Exact embeddings of a seed batch (inference.embed_nodes, sage_csr_frontier) at configs[2]'s size.

One JSON line per case.  Graph: rmat_graph(20, 16_000_000, seed=0), bench.py's configs[2] graph; table 256 wide, h1 = h2 = 128,
4096 seeds drawn without replacement.  One process; the two sides of every comparison ALTERNATE call by call inside one timed
loop (other people's work shares the machine: a drift hits both sides alike).  Times: device events around the call, which
includes the call's own host reads; median / min / max of --reps after --warmup.
  embed      embed_nodes against embed_all_nodes (gcn encoder), and that the seeds' rows are bit-equal
  frontier   ops.csr_frontier (+ clear) against the torch formulation of the same set: the seeds' CSR ranges expanded with
             repeat_interleave, the neighbours gathered, torch.unique over seeds and neighbours (int64 temporaries of E_sel entries
             and a sort); both sides are given E_sel, so neither pays for finding it
  memory     peak allocated bytes above the inputs of one embed_nodes call and of one embed_all_nodes call
Run on an MI355X: python experiments/mb_embed_nodes.py [--scale 20 --edges 16000000 --seeds 4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "graphsage-simple_amd")]

from sage355 import ops  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402
from sage355.inference import embed_all_nodes, embed_nodes  # noqa: E402


def timed_pair(fa, fb, warmup, reps):
    """fa and fb alternate; -> two (median, min, max) in seconds."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for side, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[side].append(a.elapsed_time(b) * 1e-3)
    return tuple((float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts)


def ms(t):
    return {"ms": round(t[0] * 1e3, 3), "ms_min": round(t[1] * 1e3, 3), "ms_max": round(t[2] * 1e3, 3)}


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del keep
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=16_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_embed_nodes needs an MI355X")
    g = rmat_graph(args.scale, args.edges, seed=0)
    n, nnz, d0, h = g.num_nodes, g.nnz, args.dim, args.hidden
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(n, d0, generator=gen).cuda()
    w1 = (torch.randn(h, d0, generator=gen) / d0 ** 0.5).cuda()
    w2 = (torch.randn(h, h, generator=gen) / h ** 0.5).cuda()
    rp, cl = g.to("cuda")
    seeds_np = np.random.default_rng(0).choice(n, args.seeds, replace=False)
    seeds = torch.from_numpy(seeds_np.astype(np.int32)).cuda()
    s64 = seeds.long()
    e_sel = int((rp[s64 + 1] - rp[s64]).sum())
    shape = {"graph": f"rmat({args.scale}, {args.edges})", "nodes": n, "nnz": nnz, "seeds": args.seeds, "seed_edges": e_sel}

    # (b) the frontier alone
    fr = ops.CsrFrontier(n, "cuda", max_nodes=min(n, args.seeds + e_sel))

    def kernel_form():
        ops.csr_frontier(rp, cl, seeds, fr, max_edges=e_sel)
        fr.clear()

    def torch_form():
        start = rp[s64]
        deg = rp[s64 + 1] - start
        first = torch.cumsum(deg, 0) - deg
        idx = torch.repeat_interleave(start - first, deg, output_size=e_sel) + torch.arange(e_sel, device="cuda")
        return torch.unique(torch.cat([s64, cl[idx].long()]))

    ops.csr_frontier(rp, cl, seeds, fr, max_edges=e_sel)
    size = fr.size()
    same = bool(torch.equal(torch.sort(fr.nodes[:size].long()).values, torch_form()))
    fr.clear()
    tk, tt = timed_pair(kernel_form, torch_form, args.warmup, args.reps)
    print(json.dumps({"case": "frontier", **shape, "frontier": size, "same_set": same, "csr_frontier_and_clear": ms(tk), "torch_unique": ms(tt),
                      "kernel_over_torch": round(tk[0] / tt[0], 3), "peak_MiB_kernel": round(peak_of(kernel_form) / 2 ** 20, 2),
                      "peak_MiB_torch": round(peak_of(torch_form) / 2 ** 20, 2)}), flush=True)

    # (a) the batch against the whole graph
    def few():
        return embed_nodes(rp, cl, table, w1, w2, seeds, frontier=fr)

    def every():
        return embed_all_nodes(rp, cl, table, w1, w2)

    equal = bool(torch.equal(few().view(torch.int32), every()[s64].view(torch.int32)))
    tf, ta = timed_pair(few, every, args.warmup, max(5, args.reps // 2))
    print(json.dumps({"case": "embed", **shape, "frontier": size, "d0": d0, "h1": h, "h2": h, "bit_equal": equal, "embed_nodes": ms(tf),
                      "embed_all_nodes": ms(ta), "nodes_over_all": round(tf[0] / ta[0], 3)}), flush=True)

    # (c) peak memory above the inputs (embed_nodes once with the caller's map, once building its own)
    print(json.dumps({"case": "memory", **shape, "frontier": size, "peak_MiB_embed_nodes_own_map": round(peak_of(lambda: embed_nodes(rp, cl, table, w1, w2, seeds)) / 2 ** 20, 1),
                      "peak_MiB_embed_nodes_kept_map": round(peak_of(few) / 2 ** 20, 1), "peak_MiB_embed_all_nodes": round(peak_of(every) / 2 ** 20, 1)}),
          flush=True)


if __name__ == "__main__":
    main()
