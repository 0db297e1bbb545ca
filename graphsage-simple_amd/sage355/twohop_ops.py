"""The two-layer stack (model.py:219-222) from the public operators, for any fanouts up to native.MAX_FANOUT_WIDE.

TwoHopEngine runs the stack as one C call (sage_forward2), whose samplers give a lane to each sample slot and so stop at
native.MAX_FANOUT.  This module runs the same stack operator by operator -- sample (the narrow or the wide entry, by k), frontier,
sample, gather_mean + linear_act twice -- and defines its sets exactly as the engine does, so for fanouts the engine takes the
integer sets are the engine's for the same key.  Every operator is an autograd node (autograd.py): the result is differentiable
in w1, w2 and a table that requires grad.  One host read of the frontier size per call (Frontier.size()).
"""
import torch

from . import autograd, native, ops
from .ops import ACT_RELU, TAG_INNER, TAG_INNER_SELF, TAG_OUTER


def two_hop_forward(rowptr, col, table, w1, w2, seeds, k1, k2, key, concat=False, agg_self_loop=False,
                    act1=ACT_RELU, act2=ACT_RELU, rowptr_outer=None, col_outer=None, return_sets=False):
    """seeds [B] -> out [B, h2] on the device, or (out, sets) with return_sets.

    rowptr / col: the CSR layer 1 samples from; rowptr_outer / col_outer: layer 2's, when it differs.  table [N, d0],
    w1 [h1, d0 | 2 d0], w2 [h2, h1 | 2 h1] (the reference Parameters; concat = the gcn=False encoder).  key: the 64-bit sampler key.
    The sets (TwoHopEngine's): the outer hop draws k2 neighbours of every seed with (key, TAG_OUTER) into a frontier (with the
    seed itself when agg_self_loop); the layer-1 node list is [seeds |] frontier nodes (the seeds lead it for the concat encoder,
    whose frontier rows start at B); the inner hop draws k1 neighbours with (key, TAG_INNER) for the frontier nodes and
    (key, TAG_INNER_SELF) for the concat seed rows.
    sets: nbr2, cnt2, s1_nodes, first_frontier_row, n_s1, nbr1, cnt1 -- the keys of TwoHopEngine.intermediates()."""
    k1, k2 = int(k1), int(k2)
    for name, k in (("k1", k1), ("k2", k2)):
        if not 1 <= k <= native.MAX_FANOUT_WIDE:
            raise native.SageError(f"two_hop_forward: {name} = {k} outside [1, {native.MAX_FANOUT_WIDE}]")
    dev = table.device
    num_nodes = rowptr.shape[0] - 1
    if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.is_contiguous()):
        seeds = ops.as_ids(seeds, dev, num_nodes)
    rowptr2, col2 = (rowptr, col) if rowptr_outer is None else (rowptr_outer, col_outer)
    b = seeds.shape[0]
    h1_dim, h2_dim = w1.shape[0], w2.shape[0]
    if b == 0:
        out = torch.zeros((0, h2_dim), dtype=torch.float32, device=dev)
        empty = torch.zeros((0,), dtype=torch.int32, device=dev)
        sets = {"nbr2": empty.view(0, k2), "cnt2": empty, "s1_nodes": empty, "first_frontier_row": 0, "n_s1": 0,
                "nbr1": empty.view(0, k1), "cnt1": empty}
        return (out, sets) if return_sets else out
    first = b if concat else 0
    self_loop = bool(agg_self_loop)

    # outer hop: seeds -> nbr2, every sampled id into the frontier, rows from `first` on
    frontier = ops.Frontier(b * (k2 + int(self_loop)), dev, first_row=first)
    any2 = torch.zeros(1, dtype=torch.int32, device=dev)
    nbr2, cnt2, slot2, self_slot2 = ops.sample_neighbors_any(rowptr2, col2, seeds, k2, key, TAG_OUTER, frontier=frontier,
                                                              insert_self=self_loop, any_nonempty=any2)
    n1 = frontier.size()                                   # the one host read: first + distinct ids
    if concat:
        frontier.nodes[:b] = seeds
    s1 = frontier.nodes[:n1]

    # inner hop: the layer-1 node list -> nbr1
    nbr1 = torch.empty((n1, k1), dtype=torch.int32, device=dev)
    cnt1 = torch.empty(n1, dtype=torch.int32, device=dev)
    any1 = torch.zeros(1, dtype=torch.int32, device=dev)
    if concat:
        ops.sample_neighbors_any(rowptr, col, s1[:b], k1, key, TAG_INNER_SELF, any_nonempty=any1, out_nbr=nbr1[:b], out_cnt=cnt1[:b])
    if n1 > first:
        ops.sample_neighbors_any(rowptr, col, s1[first:], k1, key, TAG_INNER, any_nonempty=any1, out_nbr=nbr1[first:], out_cnt=cnt1[first:])

    # layer 1 on the node list (encoders.py:47-62 with features = the table)
    if n1 > 0:
        agg1 = autograd.gather_mean(table, nbr1, cnt1, any1, None, s1 if self_loop else None)
        h1 = autograd.linear_act(agg1, w1, act1, table if concat else None, s1 if concat else None)
    else:
        h1 = torch.zeros((1, h1_dim), dtype=torch.float32, device=dev)    # gcn, every seed isolated: nothing below reads a row of it
    # layer 2 on the seeds: neighbours are hash slots, frontier.rows turns them into rows of h1; the concat self rows are h1[:b]
    agg2 = autograd.gather_mean(h1, slot2, cnt2, any2, frontier.rows, self_slot2 if self_loop else None)
    out = autograd.linear_act(agg2, w2, act2, h1 if concat else None, None)
    if not return_sets:
        return out
    sets = {"nbr2": nbr2, "cnt2": cnt2, "s1_nodes": s1, "first_frontier_row": first, "n_s1": n1, "nbr1": nbr1, "cnt1": cnt1}
    return out, sets
